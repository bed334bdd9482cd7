"""A reference for the pools' openings= from the pools alone: a C4SelfPlay / ChessSelfPlay (or
tests/arena_ref.py's reference arena) built WITHOUT a book, whose roots and history rows the test
itself seeds in torch from the recorder's slot table after start() and after every step().  No
zc_traj_openings_async: what the pools with a book must reproduce game for game."""
import torch


def as_rows(book) -> torch.Tensor:
    """A book ([N, 3] int64 or [N, 72] uint8) as [N, W] int64 rows."""
    return book.contiguous().view(torch.int64) if book.dtype == torch.uint8 else book.contiguous()


def fresh_slots(pool) -> torch.Tensor:
    """The slots whose game has only its first position."""
    slot = pool.traj.slot
    return (slot[:, 1] >= 0) & (slot[:, 0] == 1)


def seed(pool, book: torch.Tensor, share: int):
    """The rule in torch: slot g with game number `game` >= 0 and one position takes row
    (game // share) % N as its root and its history's position 0."""
    rows = as_rows(book).to(pool.dev)
    fresh = fresh_slots(pool)
    game = pool.traj.slot[:, 1].to(torch.int64).clamp(min=0)
    pick = rows[(game // share) % rows.shape[0]]
    roots = pool.roots.view(torch.int64) if pool.roots.dtype == torch.uint8 else pool.roots
    roots[fresh] = pick[fresh]
    pool.traj.hist[fresh, 0] = pick[fresh]


def play(pool, total_games: int, after_step=None, on_search=None, max_steps: int = 2000):
    """selfplay.simulate_games with `after_step(pool)` after start() and after every step(), and
    `on_search(pool, fresh)` between a step's search and its play (fresh: the slots at a game's
    first position, as the search found them).  Returns the batch's tensors on the host."""
    pool.start(total_games)
    if after_step:
        after_step(pool)
    steps = 0
    while total_games and (steps % 4 or pool.traj.finished() < total_games):
        assert steps < max_steps, f"{pool.traj.finished()} of {total_games} games finished in {max_steps} steps"
        fresh = fresh_slots(pool).clone()
        pool.traj.ensure_room()
        pool.step_search()
        if on_search:
            on_search(pool, fresh)
        pool.step_finish()
        if after_step:
            after_step(pool)
        steps += 1
    pool.last_batch = b = pool.take()
    assert b.games.shape[0] == total_games
    return b.rows.cpu(), b.labels.cpu(), b.moves.cpu(), b.games.cpu()


def first_rows(games_batch) -> torch.Tensor:
    """Every game's first row, in game-number order."""
    rows, _, _, games = games_batch
    return rows[games[:, 3]]
