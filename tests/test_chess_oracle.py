"""The chess oracle (oracle/chess_oracle.c) against the reference's own outputs
(tests/golden/chess_*.json, generated from engine/games/chess compiled unmodified)."""
import numpy as np
import pytest

import oracle


def test_perft_matches_reference(golden):
    for case in golden("chess_perft.json")["perft"]:
        s = oracle.chess_from_fen(case["fen"])
        for d, n in enumerate(case["counts"], start=1):
            assert oracle.chess_perft(s, d) == n, (case["name"], d)


def test_perft_start_depth5():
    assert oracle.chess_perft(oracle.chess_init(), 5) == 4865351


def test_ordered_move_lists_with_capture_values(golden):
    cases = golden("chess_movelists.json")["cases"]
    assert len(cases) >= 250
    for case in cases:
        got = oracle.chess_moves(oracle.chess_from_json(case["state"]))
        assert [list(m) for m in got] == case["moves"]


def test_play_move(golden):
    for case in golden("chess_play.json")["cases"]:
        s = oracle.chess_from_json(case["state"])
        o = oracle.chess_play(s, case["move"])
        a = case["after"]
        assert bytes(o.board).decode("latin-1") == a["board"]
        b = case["state"]   # the fixture's "before" state carries only its history lengths
        assert (o.turn, o.fifty, o.castle) == (a["turn"], a["fifty"], a["castle"])
        assert (o.nhw, o.nhb) == (a["nhw"] - b["nhw"], a["nhb"] - b["nhb"])
        mv = case["move"]
        head = "%d%d%d%d%d" % (mv[0], mv[1], mv[2], mv[3], int(mv[4]))
        assert (a["hw_head"] if s.turn == 0 else a["hb_head"]) == head


def test_terminal_flags(golden):
    cases = golden("chess_terminal.json")["cases"]
    assert sum(c["win"] for c in cases) >= 10 and sum(c["draw"] for c in cases) >= 20
    for case in cases:
        s = oracle.chess_from_json(case["state"])
        assert oracle.chess_win(s) == case["win"], case.get("note", case.get("fen"))
        assert oracle.chess_draw(s) == case["draw"], case.get("note", case.get("fen"))
        if "expect" in case:  # the reference's own test expectations (tests/test_cb.py:105-116)
            assert [case["win"], case["draw"]] == case["expect"]


def test_state_to_tensor(golden):
    for case in golden("chess_tensor.json")["cases"]:
        t = oracle.chess_tensor(oracle.chess_from_json(case["state"]))
        bits = np.unpackbits(np.frombuffer(bytes.fromhex(case["bits"]), np.uint8))[: 17 * 64]
        np.testing.assert_array_equal((t.reshape(-1) != 0).astype(np.uint8), bits)
        assert list(t.shape) == case["shape"]


def test_chess_search_matches_reference(golden):
    """Chess get_move (crude_chess_score, immediate_value / random policy) vs the reference."""
    _check_get_move(golden("chess_get_move.json")["cases"])


def test_chess_search_at_the_engine_limits(golden):
    """The reference at the limits the engine declares (tests/golden/gen_golden_limits.py):
    flushes of 129 and 256 leaves, and 65533 simulations, where node ids pass 15 bits."""
    cases = golden("chess_get_move_limits.json")["cases"]
    assert {(c["sims"], c["bs"]) for c in cases} >= {(400, 129), (400, 256), (65533, 64), (65533, 256)}
    _check_get_move(cases)


def _check_get_move(cases):
    for case in cases:
        s = oracle.chess_from_fen(case["fen"])
        mt = oracle.MT(case["seed"])
        best, moves, na = oracle.chess_get_move(s, mt, case["sims"], case["c"], case["bs"], case["policy"],
                                                case["freedom"])
        assert [list(m) for m in moves] == case["root_moves"]
        assert na == case["root_na"], case["fen"]
        assert list(moves[best]) == case["move"]
        assert mt.drawn == case["consumed"]
        assert mt.u32() == case["next_word"]


def test_chess_selfplay_batch_equals_get_move_play_judge():
    """zcc_selfplay_batch (bench.py's chess CPU baseline) = per game, per move: get_move
    (crude_chess_score, immediate_value(3)), play the best move, refill at a finished game —
    the same stream consumption as the step-by-step oracle calls, from mixed positions."""
    import copy
    import numpy as np
    rng = np.random.default_rng(3)
    states = []
    for _ in range(6):
        s = oracle.chess_init()
        for _ in range(int(rng.integers(0, 30))):
            ms = oracle.chess_moves(s)
            if not ms or oracle.chess_draw(s):
                break
            s = oracle.chess_play(s, ms[int(rng.integers(len(ms)))])
        states.append(s)
    rows = np.zeros((len(states), 72), np.uint8)
    for i, s in enumerate(states):
        rows[i, :64] = list(s.board)
        rows[i, 64:67] = (s.turn, s.fifty, s.castle)
    mts = [oracle.MT(40 + i) for i in range(len(states))]
    ref = [copy.deepcopy(m) for m in mts]
    K, S = 5, 60
    exp = oracle.chess_selfplay_batch(rows, mts, K, S, 1.4, 16, threads=3)
    assert (exp > 0).all() and (exp <= K * S).all()
    for i, s in enumerate(states):
        s = oracle.chess_state(bytes(rows[i, :64]).decode("latin-1"), int(rows[i, 64]), int(rows[i, 65]),
                               int(rows[i, 66]))
        for _ in range(K):
            best, ms, _ = oracle.chess_get_move(s, ref[i], S, 1.4, 16, "immediate_value", 3.0)
            s = oracle.chess_play(s, ms[best])
            if not oracle.chess_moves(s) or oracle.chess_draw(s):
                s = oracle.chess_init()
        assert ref[i].state() == mts[i].state(), i


# A ring of queens round an empty centre: more legal moves than any list holds (no game reaches it).
QUEEN_RING = "KQQQQQQQQ      QQ      QQ      QQ      QQ      QQ      QQQQQQQQk"
WIDEST = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"   # 218 legal moves, the most of a legal position


def _pseudo_moves(board, t):
    """(from, to) of side t's pseudo-legal queen, rook, bishop, knight and king moves on `board`
    (no pawns): every target that is empty or an enemy piece other than the king."""
    mine = (lambda x: x.isupper()) if t == 0 else (lambda x: x.islower())
    diag, orth = [(-1, -1), (-1, 1), (1, -1), (1, 1)], [(-1, 0), (1, 0), (0, -1), (0, 1)]
    knight = [(-2, -1), (-2, 1), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, -1), (2, 1)]
    out = []
    for s, x in enumerate(board):
        if x == " " or not mine(x):
            continue
        u = x.upper()
        for dr, dc in {"B": diag, "R": orth, "Q": diag + orth, "K": diag + orth, "N": knight}[u]:
            r, c = s // 8 + dr, s % 8 + dc
            while 0 <= r < 8 and 0 <= c < 8:
                y = board[r * 8 + c]
                if y == " " or (not mine(y) and y.upper() != "K"):
                    out.append((s, r * 8 + c))
                if y != " " or u in "KN":
                    break
                r, c = r + dr, c + dc
    return out


def _king_attacked(board, t):
    """Is side t's king attacked on `board`?  A king is never a target, so a queen of its colour
    stands in for it and the other side's pseudo-legal targets are asked for its square."""
    k = board.index("K" if t == 0 else "k")
    probe = board[:k] + ("Q" if t == 0 else "q") + board[k + 1:]
    return any(to == k for _, to in _pseudo_moves(probe, 1 - t))


def test_more_moves_than_a_list_holds_raise():
    """A board with more legal moves than ZCC_MAX_MOVES: `chess_moves` refuses, and so does every
    caller that keeps a list (get_move: OverflowError, perft below depth 1: 2^64 - 1, the
    rollout: 3); the terminal tests, which only ask whether a move exists, answer."""
    s = oracle.chess_state(QUEEN_RING)
    with pytest.raises(OverflowError, match="277"):
        oracle.chess_moves(s)
    with pytest.raises(OverflowError):
        oracle.chess_get_move(s, oracle.MT(1), 8, 1.4, 4)
    assert oracle.chess_perft(s, 1) == 277 and oracle.chess_perft(s, 2) == 2 ** 64 - 1
    assert oracle.chess_rollout(s, oracle.MT(1)) == (3, 0)
    assert not oracle.chess_win(s) and not oracle.chess_draw(s)


def test_more_moves_than_a_list_holds_are_counted():
    """The true count: the pseudo-legal moves less those after which the mover's king is attacked
    (the oracle's `chess_play`, then the attack read off the board)."""
    from test_gpu_chess import _count_runs
    s = oracle.chess_state(QUEEN_RING)
    pseudo = _pseudo_moves(QUEEN_RING, 0)
    assert len(pseudo) == _count_runs(list(QUEEN_RING), 0)[1] == 277
    rejected = 0
    for f, t in pseudo:
        after = oracle.chess_play(s, (f // 8, f % 8, t // 8, t % 8, 0.0))
        rejected += _king_attacked(bytes(after.board).decode("latin-1"), 0)
    n = oracle.chess_move_count(s)
    assert n > oracle.ZCC_MAX_MOVES and n == len(pseudo) - rejected == 277
    # a pinned queen: the count drops by the moves that leave the pin's line
    pinned = "KQr" + QUEEN_RING[3:]
    m = oracle.chess_move_count(oracle.chess_state(pinned))
    want = sum(not _king_attacked(bytes(oracle.chess_play(oracle.chess_state(pinned), (f // 8, f % 8, t // 8, t % 8, 0.0))
                                       .board).decode("latin-1"), 0) for f, t in _pseudo_moves(pinned, 0))
    assert m == want < len(_pseudo_moves(pinned, 0))


def test_the_widest_legal_position_still_returns_its_list():
    s = oracle.chess_from_fen(WIDEST)
    moves = oracle.chess_moves(s)
    assert len(moves) == oracle.chess_move_count(s) == 218
    assert len({m[:4] for m in moves}) == 218
    assert oracle.chess_perft(s, 1) == 218
