"""Connect4 root positions for the GPU parity tests (42-char boards, row 0 at the top, and the
side to move), drawn from a caller's random.Random so that each test keeps its own set."""
import oracle

EMPTY = "." * 42


def opening(rng, max_plies):
    """A position 0..max_plies random plies from the empty board (won ones included)."""
    b, t = EMPTY, 0
    for _ in range(rng.randint(0, max_plies)):
        legal = [col for col in range(7) if b[col] == "."]
        b, t = oracle.play(b, t, rng.choice(legal))
    return b, t


def deep_leaning_roots(rng, n):
    """n roots 18 to 41 plies deep from games that lean on one to three columns, so that the
    search's chains meet full columns and full boards; a few already-won roots stay (get_move
    still searches them), drawn boards do not."""
    boards = []
    while len(boards) < n:
        b, t = EMPTY, 0
        lean = rng.sample(range(7), rng.randint(1, 3))  # columns filled first: chains hit full columns
        ok = True
        for _ in range(rng.randint(18, 41)):
            legal = [col for col in range(7) if b[col] == "."]
            pref = [col for col in legal if col in lean]
            b, t = oracle.play(b, t, rng.choice(pref if pref and rng.random() < 0.7 else legal))
            if oracle.check_win(b, t):
                ok = rng.random() < 0.1  # a few already-won roots stay (get_move still searches them)
                break
        if ok and not oracle.check_draw(b):
            boards.append((b, t))
    return boards


def states(boards):
    """[(board, turn)] -> zc_c4_state records."""
    import numpy as np
    from zeroclone_amd._native import C4_STATE_DTYPE, c4_from_rows
    out = np.zeros(len(boards), C4_STATE_DTYPE)
    for i, (b, t) in enumerate(boards):
        out[i] = c4_from_rows(b, t)
    return out
