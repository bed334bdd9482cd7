"""Pin the CPU restatement (oracle/) to the reference's own outputs (tests/golden/)."""
import pytest

import oracle


def test_mt19937_known_answers(golden):
    kat = golden("mt19937_kat.json")
    seed0 = kat["seed0_state"]
    m = oracle.MT(0)
    st, idx = m.state()
    assert st == seed0[:624] and idx == seed0[624]
    for e in kat["seeds"]:
        m = oracle.MT(e["seed"])
        assert [m.u32() for _ in range(16)] == e["getrandbits32"]
        m = oracle.MT(e["seed"])            # one stream, consumed in the fixture's n order
        for n, vals in e["randbelow"].items():
            assert [m.randbelow(int(n)) for _ in range(len(vals))] == vals, (e["seed"], n)


def test_set_order_matches_cpython(golden):
    order = golden("c4_set_order.json")["order"]
    assert len(order) == 128
    for mask, cols in order.items():
        assert oracle.set_order(int(mask)) == cols


def test_backend_rules(golden):
    for c in golden("c4_backend.json")["cases"]:
        assert oracle.check_win(c["board"], c["turn"]) == c["win"]
        assert oracle.check_draw(c["board"]) == c["draw"]


def test_rollouts(golden):
    for c in golden("c4_rollout.json")["cases"]:
        assert oracle.rollout(c["board"], c["turn"], c["seed"]) == (c["value"], c["consumed"])


def test_get_move_root_visits(golden):
    cases = golden("c4_get_move.json")["cases"]
    assert len(cases) >= 100
    for c in cases:
        col, na, order, used = oracle.get_move(c["board"], c["turn"], c["seed"], c["sims"], c["c"], c["bs"])
        assert order == c["order"]
        assert na == c["root_na"], (c["seed"], c["sims"], c["bs"])
        assert col == c["move"]
        assert used == c["consumed"]


def test_get_move_at_the_engine_limits(golden):
    """The reference at the limits the engine declares (tests/golden/gen_golden_limits.py):
    batch sizes 128 to 512, either side of the search kernel's 314 / 315 workgroup boundary, and
    65533 simulations, where node ids pass 15 bits."""
    cases = golden("c4_get_move_limits.json")["cases"]
    shapes = {(c["sims"], c["bs"]) for c in cases}
    assert shapes >= {(1100, 128), (1100, 314), (1100, 315), (1100, 512), (65533, 32), (65533, 512)}
    for c in cases:
        mt = oracle.MT(c["seed"])
        col, na, order = oracle.get_move_mt(c["board"], c["turn"], mt, c["sims"], c["c"], c["bs"])
        assert order == c["order"]
        assert na == c["root_na"], (c["seed"], c["sims"], c["bs"])
        assert col == c["move"]
        assert mt.drawn == c["consumed"]
        assert mt.u32() == c["next_word"]


def test_batch_matches_single(golden):
    cases = [c for c in golden("c4_get_move.json")["cases"] if c["sims"] == 100][:16]
    mv, na, cons = oracle.get_move_batch([c["board"] for c in cases], [c["turn"] for c in cases],
                                         [c["seed"] for c in cases], 100, 1.4, 32, threads=4)
    for i, c in enumerate(cases):
        if c["bs"] != 32 or c["c"] != 1.4:
            continue
        assert mv[i] == c["move"]
        assert [int(na[i][col]) for col in c["order"]] == c["root_na"]
        assert cons[i] == c["consumed"]


def test_selfplay_stream_continues_across_moves(golden):
    for g in golden("c4_selfplay.json")["games"]:
        mt = oracle.MT(g["seed"])
        board, turn = "." * 42, 0
        moves = []
        while not (oracle.check_win(board, turn) or oracle.check_draw(board)):
            col, _, _ = oracle.get_move_mt(board, turn, mt, g["sims"], g["c"], g["bs"])
            moves.append(col)
            board, turn = oracle.play(board, turn, col)
        assert moves == g["moves"]
        result = (turn * 2 - 1) if oracle.check_win(board, turn) else 0
        assert result == g["result"]
        assert mt.drawn == g["consumed"]
