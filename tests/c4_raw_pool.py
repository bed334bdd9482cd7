"""A Connect4 engine with the device buffers of its self-play launches, called by hand (the C ABI's
view: any first_game, root buffer and parameters), for the tests that go where C4SelfPlay never
takes the engine.  Every launch pre-fills its outputs with a pattern, so a test sees exactly what
a launch wrote — or that a refused call wrote nothing."""
import numpy as np
import torch

from zeroclone_amd import _native

ONGOING, SKIP = 2, 4
OK, NO_MOVES, BAD_STATE, INTERNAL, CAPACITY = 0, 1, 2, 3, 4
FILL64, FILL32, FILL16 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A5A
# zc_game_stats as int64 columns
EXPANSIONS, DEPTH_SUM, LEAVES, PLIES, RNG_WORDS, STATUS, BLOCKS, RESERVED = range(8)


def c4_rows(states) -> torch.Tensor:
    """zc_c4_state records (numpy C4_STATE_DTYPE) as [n, 3] int64 device rows."""
    a = np.ascontiguousarray(states, dtype=_native.C4_STATE_DTYPE)
    return torch.from_numpy(a.view(np.int64).reshape(len(a), 3).copy()).cuda()


def raw_state(stones0: int, stones1: int, turn: int, reserved: int = 0) -> np.void:
    """A zc_c4_state from its fields, valid or not."""
    out = np.zeros((), _native.C4_STATE_DTYPE)
    out["stones"] = (stones0, stones1)
    out["turn"] = turn
    out["reserved"] = reserved
    return out


class RawPool:
    def __init__(self, games: int, max_sims: int, max_batch: int, seeds, steps_cap: int):
        self.eng = _native.NativeEngine(max_games=games, max_sims=max_sims, max_batch=max_batch)
        self.eng.seed(0, list(seeds))
        self.G, self.cap = games, steps_cap
        dev = "cuda"
        self.roots = torch.zeros((games, 3), dtype=torch.int64, device=dev)
        self.states = torch.empty(steps_cap * games * 3, dtype=torch.int64, device=dev)
        self.moves = torch.empty(steps_cap * games, dtype=torch.int16, device=dev)
        self.results = torch.empty(steps_cap * games, dtype=torch.int32, device=dev)
        self.stats = torch.empty((games, 8), dtype=torch.int64, device=dev)
        self.ticket = torch.empty(2, dtype=torch.int32, device=dev)
        self.fill()

    def close(self):
        torch.cuda.synchronize()
        self.eng.close()

    def fill(self):
        self.states.fill_(FILL64)
        self.moves.fill_(FILL16)
        self.results.fill_(FILL32)
        self.stats.fill_(FILL64)
        self.ticket.fill_(FILL32)
        torch.cuda.synchronize()

    def untouched(self) -> bool:
        """After a stream synchronise: every output still holds its fill pattern."""
        torch.cuda.synchronize()
        return all(bool((x == v).all()) for x, v in ((self.states, FILL64), (self.moves, FILL16),
                                                     (self.results, FILL32), (self.stats, FILL64),
                                                     (self.ticket, FILL32)))

    def launch(self, form: str, moves: int, sims: int, bs: int, c: float = 1.4, first: int = 0, n: int | None = None,
               roots_ptr: int | None = None, budget: int | None = None):
        """One self-play launch, "free" / "pooled" / "carry", over games [first, first + n) with
        root rows at roots_ptr (default: this pool's rows of those games); synchronised."""
        n = self.G - first if n is None else n
        assert moves <= self.cap and n <= self.G
        self.fill()
        rp = self.roots.data_ptr() + 24 * first if roots_ptr is None else roots_ptr
        outs = (self.states.data_ptr(), self.moves.data_ptr(), self.results.data_ptr(), self.stats.data_ptr())
        if form == "free":
            self.eng.c4_selfplay_async(rp, n, sims, c, bs, moves, *outs, first_game=first)
        else:
            self.eng.c4_selfplay_pooled_async(rp, n, sims, c, bs, moves, n * moves if budget is None else budget,
                                              self.ticket.data_ptr(), *outs, first_game=first,
                                              carry=form == "carry")
        torch.cuda.synchronize()
        return self.rows(moves, n)

    def tables(self, moves: int, n: int):
        """The launch's [moves][n] outputs on the host: results, moves, states."""
        return (self.results[:moves * n].view(moves, n).cpu(), self.moves[:moves * n].view(moves, n).cpu(),
                self.states[:moves * n * 3].view(moves, n, 3).cpu())

    def rows(self, moves: int, n: int):
        """Per game of the launch, its finished moves in step order: (result, move, state)."""
        res, mv, st = self.tables(moves, n)
        played = res != SKIP
        m = played.sum(0)
        assert torch.equal(played, torch.arange(moves)[:, None] < m[None, :])   # a prefix of the steps
        assert bool((mv[~played] == -1).all())
        return [[(int(res[j, g]), int(mv[j, g]), st[j, g].tolist()) for j in range(int(m[g]))] for g in range(n)]

    def rng(self, g: int):
        mt, idx = self.eng.get_rng_state(g)
        return mt.tolist(), idx
