"""Dead leaves (the last mover already has four: value -1; the board is full: value 0) take no
turn of the rollouts' serial loop: their values come from the lane-parallel setup, they consume
no word and count no ply or block.  Engine.c4_rollouts on hand-built state lists against the
oracle's rollout replayed in order on the same MT state (values, words consumed, the final RNG
state), and searches from roots whose trees exhaust or end at once, through the lockstep kernel
(against oracle.get_move_mt) and through a one-move self-play launch (against the lockstep
kernel: a dead leaf adds nothing to rollout_plies / rollout_blocks in either)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

# a whole game without a four for either side: its 42 moves fill the board (a draw), and every
# prefix is a position nobody has won
DRAWN_GAME = [5, 4, 5, 0, 6, 2, 4, 5, 5, 0, 4, 1, 1, 0, 4, 5, 6, 5, 3, 1, 1, 2, 2, 6, 2, 6, 6, 3, 6, 2, 0, 3, 0, 3, 3,
              4, 3, 1, 4, 2, 1, 0]


def after(moves):
    b, t = "." * 42, 0
    for col in moves:
        assert not oracle.check_win(b, t)
        b, t = oracle.play(b, t, col)
    return b, t


def dead_states():
    won = after([0, 1, 0, 1, 0, 1, 0])   # X stacked four in column 0; O to move
    full = after(DRAWN_GAME)
    assert oracle.check_win(*won) and not oracle.check_draw(won[0])
    assert oracle.check_draw(full[0]) and not oracle.check_win(*full)
    return [won, full]


def live_states():
    rng = random.Random(5)
    out = [after(DRAWN_GAME[:k]) for k in (0, 7, 20, 33, 39, 41)]   # 41: one cell left
    while len(out) < 11:
        b, t = "." * 42, 0
        for _ in range(rng.randint(1, 30)):
            nb, nt = oracle.play(b, t, rng.choice([c for c in range(7) if b[c] == "."]))
            if oracle.check_win(nb, nt) or oracle.check_draw(nb):
                break
            b, t = nb, nt
        out.append((b, t))
    for b, t in out:
        assert not oracle.check_win(b, t) and not oracle.check_draw(b)
    return out


PATTERNS = {   # lane -> dead?
    "all dead": lambda i, n: True,
    "all live": lambda i, n: False,
    "one live first, then dead": lambda i, n: i > 0,
    "dead first, then live": lambda i, n: i < (n + 1) // 2,
    "alternating": lambda i, n: i % 2 == 1,
    "dead at lanes 0, 31, 63, 64": lambda i, n: i in (0, 31, 63, 64),
    "the second group of 64 dead": lambda i, n: 64 <= i < 128,
}


def to_states(boards):
    from zeroclone_amd._native import C4_STATE_DTYPE, c4_from_rows
    out = np.zeros(len(boards), C4_STATE_DTYPE)
    for i, (b, t) in enumerate(boards):
        out[i] = c4_from_rows(b, t)
    return out


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=16, max_sims=64, max_batch=70)
    yield e
    e.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_rollouts_with_dead_states(eng, n, pattern):
    dead, live = dead_states(), live_states()
    boards = [dead[i % 2] if PATTERNS[pattern](i, n) else live[i % len(live)] for i in range(n)]
    seed = 1000 + n
    mt = oracle.MT(seed)
    exp = [oracle.lib().zco_rollout(b.encode(), t, ctypes.byref(mt.s)) for b, t in boards]
    for (b, t), v in zip(boards, exp):
        if oracle.check_win(b, t):
            assert v == -1
        elif oracle.check_draw(b):
            assert v == 0
    eng.seed(2, [seed])
    got, words = eng.c4_rollouts(to_states(boards), game=2)
    assert [int(x) for x in got] == exp
    assert words == mt.drawn
    state, idx = eng.get_rng_state(2)
    omt, oidx = mt.state()
    assert idx == oidx and list(state) == list(omt)


def search_roots():
    roots = [after(DRAWN_GAME[:42 - k]) for k in (1, 2, 3)]        # the tree exhausts; whole flushes are dead
    roots.append(after([0, 1, 0, 1, 0, 1]))                       # X to move wins at once (column 0)
    roots.append(after([6, 2, 6, 3, 0, 4]))                       # O's open three: O wins after any reply
    return roots


@pytest.mark.parametrize("bs", [1, 32, 63, 64, 70])
def test_searches_from_roots_that_end_at_once(eng, bs):
    from zeroclone_amd.selfplay import C4SelfPlay
    sims, seed0 = 64, 40
    roots = search_roots()
    G = len(roots)
    # the lockstep kernel against the oracle
    eng.seed(0, [seed0 + g for g in range(G)])
    mv, na, st = eng.c4_search(to_states(roots), sims, 1.4, bs)
    for g, (b, t) in enumerate(roots):
        mt = oracle.MT(seed0 + g)
        col, root_na, order = oracle.get_move_mt(b, t, mt, sims, 1.4, bs)
        assert int(mv[g]) == col, g
        by_col = [0] * 7
        for c, v in zip(order, root_na):
            by_col[c] = v
        assert [int(x) for x in na[g]] == by_col, g
        state, idx = eng.get_rng_state(g)
        omt, oidx = mt.state()
        assert idx == oidx and list(state) == list(omt), g
        assert int(st[g]["rng_words"]) == mt.drawn
        mt2 = oracle.MT(seed0 + g)   # the same search once more, for its expansions
        exp = oracle.selfplay_batch([b], [t], [mt2], 1, sims, 1.4, bs)
        assert mt2.drawn == mt.drawn
        assert int(st[g]["expansions"]) == int(exp[0]), g
        assert int(st[g]["leaves"]) == sims and int(st[g]["status"]) == 0
    # the tree of a root with k empty cells holds at most 1 + k + k (k-1) + ... nodes: dead flushes
    assert int(st[0]["expansions"]) == 1 and int(st[1]["expansions"]) <= 4 and int(st[2]["expansions"]) <= 15
    # the same searches as a one-move self-play launch
    sp = C4SelfPlay(G, sims, batch_size=bs, seed=seed0)
    sp.roots.copy_(torch.from_numpy(np.array([[int(s["stones"][0]), int(s["stones"][1]), int(s["turn"])]
                                              for s in to_states(roots)], dtype=np.int64)))
    sp.run(1)
    stats = sp.stats.cpu().numpy()
    assert sp._run_moves[0].cpu().tolist() == [int(x) for x in mv]
    for k, name in ((0, "expansions"), (1, "depth_sum"), (2, "leaves"), (3, "rollout_plies"), (4, "rng_words"),
                    (5, "status"), (6, "rollout_blocks")):
        assert stats[:, k].tolist() == [int(x) for x in st[name]], name
    for g in range(G):
        assert sp.eng.get_rng_state(g)[0].tolist() == eng.get_rng_state(g)[0].tolist()
    sp.close()
