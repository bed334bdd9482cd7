"""GPU parity of the chess rules (chess.hip) with the reference's outputs
(tests/golden/chess_*.json from engine/games/chess compiled unmodified): perft counts,
ordered legal-move lists with capture values, play_move, terminal flags, planes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAXM = 256


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=1, max_sims=1, max_batch=1)
    yield e
    e.close()


def states_from_json(cases):
    from zeroclone_amd._native import CHESS_STATE_DTYPE
    a = np.zeros(len(cases), CHESS_STATE_DTYPE)
    for i, e in enumerate(cases):
        a[i]["board"] = np.frombuffer(e["board"].encode("latin-1"), np.uint8)
        a[i]["turn"], a[i]["fifty"], a[i]["castle"] = e["turn"], e["fifty"], e["castle"]
    return a


def dev(a: np.ndarray):
    return torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).cuda()


def legal(eng, st):
    n = st.shape[0]
    moves = torch.zeros((n, MAXM), dtype=torch.int16, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    eng.chess_legal_moves_async(n, st.data_ptr(), moves.data_ptr(), counts.data_ptr())
    torch.cuda.synchronize()
    return moves.cpu().numpy().view(np.uint16), counts.cpu().numpy()


def decode(m):
    from zeroclone_amd._native import unpack_chess_move
    (fr, fc, tr, tc), v = unpack_chess_move(m)
    return [fr, fc, tr, tc, v]


def test_legal_move_lists_match_reference(eng, golden):
    cases = golden("chess_movelists.json")["cases"]
    st = dev(states_from_json([c["state"] for c in cases]))
    moves, counts = legal(eng, st)
    for i, c in enumerate(cases):
        assert counts[i] == len(c["moves"]), i
        assert [decode(m) for m in moves[i, :counts[i]]] == c["moves"], i


def perft(eng, root: np.ndarray, depth: int) -> int:
    from zeroclone_amd._native import CHESS_STATE_DTYPE
    front = dev(np.array([root], CHESS_STATE_DTYPE))
    for _ in range(depth - 1):
        n = front.shape[0]
        kids = torch.zeros((n * MAXM, 72), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        eng.chess_children_async(n, front.data_ptr(), kids.data_ptr(), 0, counts.data_ptr())
        keep = (torch.arange(MAXM, device="cuda")[None, :] < counts[:, None]).reshape(-1)
        front = kids[keep].contiguous()
    _, counts = legal(eng, front)
    assert (counts >= 0).all()
    return int(counts.sum())


def test_perft_matches_reference(eng, golden):
    from zeroclone_amd._native import chess_from_fen
    for case in golden("chess_perft.json")["perft"]:
        root = chess_from_fen(case["fen"])
        for d, n in enumerate(case["counts"], start=1):
            assert perft(eng, root, d) == n, (case["name"], d)


def test_play_move_matches_reference(eng, golden):
    from zeroclone_amd._native import CHESS_STATE_DTYPE, pack_chess_move
    cases = golden("chess_play.json")["cases"]
    st = dev(states_from_json([c["state"] for c in cases]))
    mv = torch.tensor([pack_chess_move(*c["move"]) for c in cases], dtype=torch.int32).to(torch.int16).cuda()
    out = torch.zeros_like(st)
    eng.chess_play_async(len(cases), st.data_ptr(), mv.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(-1).view(CHESS_STATE_DTYPE)
    for i, c in enumerate(cases):
        a = c["after"]
        assert bytes(got[i]["board"]).decode("latin-1") == a["board"], i
        assert (got[i]["turn"], got[i]["fifty"], got[i]["castle"]) == (a["turn"], a["fifty"], a["castle"]), i


def test_terminal_flags_match_reference(eng, golden):
    from zeroclone_amd._native import ZC_CHESS_FIFTY, ZC_CHESS_STALEMATE, ZC_CHESS_WIN
    from zeroclone_amd.engine.games.chess.chess_backend import has_repeated_prefix, moves_from_hist
    cases = golden("chess_terminal.json")["cases"]
    st = dev(states_from_json([c["state"] for c in cases]))
    flags = torch.zeros(len(cases), dtype=torch.int32, device="cuda")
    eng.chess_terminal_async(len(cases), st.data_ptr(), flags.data_ptr())
    f = flags.cpu().numpy()
    for i, c in enumerate(cases):
        assert bool(f[i] & ZC_CHESS_WIN) == c["win"], i
        rep = has_repeated_prefix(moves_from_hist(c["state"]["hw"])) and \
            has_repeated_prefix(moves_from_hist(c["state"]["hb"]))
        assert (bool(f[i] & (ZC_CHESS_STALEMATE | ZC_CHESS_FIFTY)) or rep) == c["draw"], i


def test_planes_match_state_to_tensor(eng, golden):
    cases = golden("chess_tensor.json")["cases"]
    st = dev(states_from_json([c["state"] for c in cases]))
    for f16 in (False, True):
        planes = torch.zeros((len(cases), 17, 8, 8), dtype=torch.float16 if f16 else torch.float32, device="cuda")
        eng.chess_planes_async(len(cases), st.data_ptr(), planes.data_ptr(), f16)
        p = planes.float().cpu().numpy()
        for i, c in enumerate(cases):
            bits = np.unpackbits(np.frombuffer(bytes.fromhex(c["bits"]), np.uint8))[: 17 * 64]
            np.testing.assert_array_equal((p[i].reshape(-1) != 0).astype(np.uint8), bits)


def test_backend_module_is_a_drop_in(golden):
    """zeroclone_amd's chess_backend (reference API, rules on the device) on the
    reference's own fixtures, including the repetition draw through move histories."""
    from zeroclone_amd.engine.games.chess import chess_backend as cb
    s = cb.create_init_state()
    assert len(cb.get_legal_moves(s)) == 20 and not cb.check_win(s) and not cb.check_draw(s)
    for c in golden("chess_movelists.json")["cases"][:40]:
        e = c["state"]
        st = cb.State(list(e["board"].encode("latin-1")), e["turn"], e["fifty"], e["castle"] & 1, e["castle"] & 2,
                      e["castle"] & 4, e["castle"] & 8, [], [])
        got = cb.get_legal_moves(st)
        assert [list(m[0]) + [m[1]] for m in got] == c["moves"]
    for c in golden("chess_terminal.json")["cases"]:
        if "fen" in c:
            st = cb.state_from_fen(c["fen"])
            assert [cb.check_win(st), cb.check_draw(st)] == c["expect"]
    # knight bounce: the repetition draw needs both histories periodic (test_cb.py style)
    s = cb.create_init_state()
    bounce = [((7, 6, 5, 5), 0.0), ((0, 6, 2, 5), 0.0), ((5, 5, 7, 6), 0.0), ((2, 5, 0, 6), 0.0)]
    draws = []
    for k in range(16):
        s = cb.play_move(s, bounce[k % 4])
        draws.append(cb.check_draw(s))
    exp = [c["draw"] for c in golden("chess_terminal.json")["cases"] if c.get("note", "").startswith("knight")]
    assert draws == exp and any(draws)
    t = cb.state_to_tensor(cb.create_init_state())
    assert t.shape == (17, 8, 8) and t[12].sum() == 64 and t[0, 6].sum() == 8


def _random_positions(n_games=60, plies=90, seed=11):
    """Positions along random games (oracle rules) from the reference tests' FENs, plus
    boards no game reaches: random piece soup, missing or doubled kings, unknown characters."""
    import oracle
    rng = np.random.default_rng(seed)
    fens = ["rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1",
            "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",
            "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1",
            "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1",
            "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8"]
    out = []
    for g in range(n_games):
        s = oracle.chess_from_fen(fens[g % len(fens)])
        for _ in range(plies):
            out.append((bytes(s.board), s.turn, s.fifty, s.castle))
            ms = oracle.chess_moves(s)
            if not ms:
                break
            s = oracle.chess_play(s, ms[rng.integers(len(ms))])
    alphabet = np.frombuffer(b"PNBRQKpnbrqk", np.uint8)
    for i in range(400):
        b = np.full(64, ord(" "), np.uint8)
        k = rng.integers(2, 24)
        sq = rng.choice(64, k, replace=False)
        b[sq] = rng.choice(alphabet, k)
        if i % 4 == 0:   # exactly one king each, as in play
            b[(b == ord("K")) | (b == ord("k"))] = ord(" ")
            ks = rng.choice(64, 2, replace=False)
            b[ks[0]], b[ks[1]] = ord("K"), ord("k")
        if i % 5 == 1:
            b[rng.integers(64)] = rng.choice(np.frombuffer(b"X.z\x00#", np.uint8))
        out.append((b.tobytes(), int(rng.integers(2)), int(rng.integers(60)), int(rng.integers(16))))
    return out


def test_random_positions_match_oracle(eng):
    """Move lists and terminal flags on ~5,000 game positions and 400 irregular boards
    (the bitboard view and the byte view of chess_device.h both exercised) vs the oracle."""
    import oracle
    from zeroclone_amd._native import CHESS_STATE_DTYPE, ZC_CHESS_FIFTY, ZC_CHESS_STALEMATE, ZC_CHESS_WIN
    pos = _random_positions()
    a = np.zeros(len(pos), CHESS_STATE_DTYPE)
    for i, (b, t, f, c) in enumerate(pos):
        a[i]["board"] = np.frombuffer(b, np.uint8)
        a[i]["turn"], a[i]["fifty"], a[i]["castle"] = t, f, c
    st = dev(a)
    moves, counts = legal(eng, st)
    flags = torch.zeros(len(pos), dtype=torch.int32, device="cuda")
    eng.chess_terminal_async(len(pos), st.data_ptr(), flags.data_ptr())
    f = flags.cpu().numpy()
    for i, (b, t, fifty, c) in enumerate(pos):
        s = oracle.chess_state(b.decode("latin-1"), t, fifty, c)
        want = [list(m) for m in oracle.chess_moves(s)]
        assert counts[i] == len(want), (i, b)
        assert [decode(m) for m in moves[i, :counts[i]]] == want, (i, b)
        assert bool(f[i] & ZC_CHESS_WIN) == oracle.chess_win(s), (i, b)
        assert bool(f[i] & (ZC_CHESS_STALEMATE | ZC_CHESS_FIFTY)) == oracle.chess_draw(s), (i, b)


def _rep_sequences(rng, count, cap):
    """Move histories (play order) rich in repeats: random over tiny alphabets, a block
    repeated 1-4 times at the recent end, runs of one value, short ones."""
    out = []
    for i in range(count):
        kind = i % 4
        n = int(rng.integers(0, cap + 1)) if kind < 3 else int(rng.integers(0, 24))
        if kind == 0:
            s = rng.integers(0, 3, n)
        elif kind == 1:
            p, r = int(rng.integers(1, 9)), int(rng.integers(1, 5))
            s = np.concatenate([rng.integers(0, 4, n), np.tile(rng.integers(0, 4, p), r)])[-n:] if n else np.zeros(0)
        elif kind == 2:
            s = np.concatenate([rng.integers(0, 2, n), np.full(int(rng.integers(0, 12)), 7)])[-n:] if n else np.zeros(0)
        else:
            s = rng.integers(0, 2, n)
        out.append(np.asarray(s, np.uint16))
    if cap > 3000:   # the kernel's whole LDS copy: full-length histories and long periods
        for i in range(count):
            p = int(rng.integers(1001, cap // 3 + 1))          # a period past 1000 that fits three times
            block = rng.integers(0, 50, p)
            if i % 8 == 1:     # exactly cap long, no structure
                s = rng.integers(0, 3, cap)
            elif i % 8 == 3:   # three copies of a long block at the recent end: a repeat
                s = np.concatenate([rng.integers(0, 50, cap - 3 * p), np.tile(block, 3)])
            elif i % 8 == 5:   # ... with one move of the middle copy changed: none through that period
                s = np.concatenate([rng.integers(0, 50, int(rng.integers(0, cap - 3 * p + 1))), np.tile(block, 3)])
                s[len(s) - p - 1 - int(rng.integers(0, p))] = 99
            elif i % 8 == 7:   # exactly cap long and periodic throughout (the oldest copy cut short)
                s = np.tile(block, cap // p + 1)[-cap:]
            else:
                continue
            out[i] = np.asarray(s, np.uint16)
    return out


@pytest.mark.parametrize("cap", [300, 4096])
def test_repetition_matches_has_repeated_prefix(cap):
    """zc_chess_repetition_async against chess_backend.has_repeated_prefix (the KMP of
    chess_backend.cpp:148-180) on 1,200 histories per side of up to 300 moves, most recent move
    first; and on 300 per side at the kernel's capacity of 4096 moves (kMaxHistory, the whole
    8 KB LDS copy), some exactly 4096 long, some repeating a block of more than 1000 moves."""
    from zeroclone_amd import _native
    from zeroclone_amd.engine.games.chess.chess_backend import has_repeated_prefix
    rng = np.random.default_rng(5)
    G = 1200 if cap == 300 else 300
    seqs = _rep_sequences(rng, 2 * G, cap)
    if cap == 4096:
        assert sum(len(s) == cap for s in seqs) >= G // 4
    hist = np.zeros((G, 2, cap), np.uint16)
    ln = np.zeros((G, 2), np.int32)
    for k, s in enumerate(seqs):
        hist[k // 2, k % 2, :len(s)] = s
        ln[k // 2, k % 2] = len(s)
    h, l = torch.from_numpy(hist.view(np.int16)).cuda(), torch.from_numpy(ln).cuda()
    out = torch.zeros(G, dtype=torch.int32, device="cuda")
    _native.check(_native.lib().zc_chess_repetition_async(G, cap, h.data_ptr(), l.data_ptr(), out.data_ptr(), None))
    got = out.cpu().numpy()
    hits = 0
    for k, s in enumerate(seqs):
        want = has_repeated_prefix([int(x) for x in s[::-1]])
        hits += want
        assert bool((got[k // 2] >> (k % 2)) & 1) == want, (k, s.tolist())
    # the cases exercise both answers (the guard scales with the number of histories)
    assert hits > 100 * G // 1200 and len(seqs) - hits > 100 * G // 1200


def _dense_boards(n=400, seed=23):
    """Boards no game reaches, crowded so that the mover has more than 128 (piece, direction)
    runs, where chess_device.h's run-parallel generator gives up and the per-piece generator
    takes over: the mover's queens and king fill most of every other rank (or file), the
    ranks between hold enemy pieces or nothing, so each queen keeps up to six directions open.
    The odd-numbered boards are thinned out, with rooks, bishops and knights among the queens
    (at most 128 runs: the run-parallel generator on the same kind of board).  Returns the
    boards and (runs, pseudo-legal moves) of each, as the device generator counts them."""
    rng = np.random.default_rng(seed)
    out, stats = [], []
    for i in range(n):
        t = int(rng.integers(2))
        fill = rng.uniform(0.8, 1.0) if i % 2 == 0 else rng.uniform(0.3, 0.6)
        par, foe_p = int(rng.integers(2)), rng.uniform(0.0, 0.5)
        b = [" "] * 64
        own_sq = [s for s in range(64) if (s // 8) % 2 == par and rng.random() < fill]
        other = [s for s in range(64) if (s // 8) % 2 != par]
        for s in own_sq:
            b[s] = "Q" if i % 2 == 0 else str(rng.choice(list("QQQQRBN")))
        b[int(rng.choice(own_sq))] = "K"
        ek = int(rng.choice(other))
        b[ek] = "K" if t == 1 else "k"
        for s in other:
            if s != ek and rng.random() < foe_p:
                b[s] = str(rng.choice(list("NBRQ")))
        if t == 0:   # the mover is white: own pieces upper case, the enemy's lower
            b = [x.lower() if s in set(other) else x for s, x in enumerate(b)]
        else:
            b = [x if s in set(other) else x.lower() for s, x in enumerate(b)]
        if i % 4 == 3:   # files instead of ranks
            b = [b[(s % 8) * 8 + s // 8] for s in range(64)]
        out.append(("".join(b).encode("latin-1"), t, int(rng.integers(40)), 0))
        stats.append(_count_runs(b, t))
    return out, stats


def _count_runs(b, t):
    """(non-empty runs, pseudo-legal moves) of side t's queens, rooks, bishops, knights and
    kings on board b: a knight's targets are one run, a slider or a king one per direction."""
    mine = (lambda x: x.isupper()) if t == 0 else (lambda x: x.islower())

    def target(r, c):
        x = b[r * 8 + c]
        return x == " " or (not mine(x) and x.upper() != "K")
    runs = moves = 0
    dirs = {"B": [(-1, -1), (-1, 1), (1, -1), (1, 1)], "R": [(-1, 0), (1, 0), (0, -1), (0, 1)]}
    dirs["Q"] = dirs["K"] = dirs["B"] + dirs["R"]
    for s in range(64):
        x = b[s]
        if x == " " or not mine(x):
            continue
        r, c, u = s // 8, s % 8, x.upper()
        if u == "N":
            k = sum(0 <= r + dr < 8 and 0 <= c + dc < 8 and target(r + dr, c + dc)
                    for dr, dc in ((-2, -1), (-2, 1), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, -1), (2, 1)))
            runs, moves = runs + (k > 0), moves + k
            continue
        for dr, dc in dirs[u]:
            rr, cc, k = r + dr, c + dc, 0
            while 0 <= rr < 8 and 0 <= cc < 8 and target(rr, cc):
                k += 1
                if b[rr * 8 + cc] != " " or u == "K":
                    break
                rr, cc = rr + dr, cc + dc
            runs, moves = runs + (k > 0), moves + k
    return runs, moves


# Boards at and above the generator's capacity of 256 legal moves (white to move; found by a
# hill-climb from the ring of queens, one queen removed, added or moved at a time).  Name:
# (board, legal moves, runs of the run-parallel generator).  The boards without a white king go
# through the byte view, whose generator is always the per-piece one; every pseudo-legal move of
# theirs is legal (find_king gives -1, -1).
QUEEN_RING = "KQQQQQQQQ      QQ      QQ      QQ      QQ      QQ      QQQQQQQQk"
CAPACITY_BOARDS = {
    "218": ("KQQQ QQQQ  Q   Q   Q    Q   Q  QQ      Q   Q      QQ    QQQQQ Qk", 218, 80),
    "230": ("KQQQQQQ Q      Q Q Q   QQ   Q  QQ      QQ  Q    Q Q     QQQ Q Qk", 230, 90),
    "256": ("KQQQQQQQQ      Q       QQ      QQ      QQ  Q Q QQ Q    QQQQQQQQk", 256, 82),
    "257": ("KQQQQQQQQ      Q       QQ      QQ      QQ  Q   QQ Q    QQQQQQQQk", 257, 74),
    "ring": (QUEEN_RING, 277, 67),
    "200, 129 runs": ("KQ  Q QQ   Q  Q QQQ Q Q   Q Q Q Q Q    Q  Q QQ  Q Q   QQQ Q  Q k", 200, 129),
    "227, 129 runs": ("K Q Q Q   Q Q Q QQ     Q   Q Q QQQ   Q Q   Q Q QQ Q    QQpQbQQQk", 227, 129),
    "256, no king": ("QQQQQQQQQ      Q       QQ      QQ      QQ Q  Q Q Q     Q QQQQ Qk", 256, 81),
    "257, no king": (" QQQQQQQQ      QQ      QQ      QQ      QQ Q    QQ  Q  QQQQQQQ Qk", 257, 76),
    "ring, no king": ("Q" + QUEEN_RING[1:], 282, 67),
}
ORDINARY = ["rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1",
            "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",
            "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1",
            "4k3/8/8/8/8/8/4r3/4K3 w - - 0 1"]


def _capacity_positions():
    """(name, oracle state) with every capacity board, for white and (colours swapped, the board
    turned upside down) for black, between ordinary positions."""
    import oracle
    out = []
    k = 0
    for name, (b, n, runs) in CAPACITY_BOARDS.items():
        assert _count_runs(list(b), 0)[0] == runs, name
        for t in (0, 1):
            out.append(("ordinary", oracle.chess_from_fen(ORDINARY[k % len(ORDINARY)])))
            k += 1
            bb = b if t == 0 else "".join(b[(7 - i // 8) * 8 + i % 8] for i in range(64)).swapcase()
            s = oracle.chess_state(bb, t, 3, 0)
            assert oracle.chess_move_count(s) == n, (name, t)
            out.append((name, s))
    out.append(("ordinary", oracle.chess_from_fen(ORDINARY[0])))
    return out


def _states(sts):
    from zeroclone_amd._native import CHESS_STATE_DTYPE
    a = np.zeros(len(sts), CHESS_STATE_DTYPE)
    for i, s in enumerate(sts):
        a[i]["board"] = np.frombuffer(bytes(s.board), np.uint8)
        a[i]["turn"], a[i]["fifty"], a[i]["castle"] = s.turn, s.fifty, s.castle
    return a


def test_the_generator_at_and_above_its_capacity(eng):
    """256 legal moves fit, 257 are refused with a count of -1 and nothing written: through
    zc_chess_legal_moves_async, zc_chess_children_async and the lazy-node probe, for the
    run-parallel generator (at most 128 runs), the per-piece one above 128 runs (below the
    capacity: no board with more than 128 runs and more than 256 legal moves was found) and the
    byte view's, the over-capacity positions between ordinary ones in one launch.  (The refusal of
    more than 512 pseudo-legal moves stays unexecuted: the search's best board had 282.)  Every output
    is pre-filled: an over-capacity position's own rows keep the fill, and so do the slots past a
    neighbour's list."""
    import oracle
    pos = _capacity_positions()
    n = len(pos)
    want_n = [oracle.chess_move_count(s) for _, s in pos]
    assert {256, 257, 277} <= set(want_n) and any(192 < w < 256 for w in want_n)
    st = dev(_states([s for _, s in pos]))
    FILL = 0x5A5A
    moves = torch.full((n, MAXM), FILL, dtype=torch.int16, device="cuda")
    counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    kids = torch.full((n * MAXM, 72), 0xA5, dtype=torch.uint8, device="cuda")
    kmoves = torch.full((n, MAXM), FILL, dtype=torch.int16, device="cuda")
    kcounts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    kids2 = torch.full((n * MAXM, 72), 0xA5, dtype=torch.uint8, device="cuda")
    k2counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    probe = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    flags = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    eng.chess_legal_moves_async(n, st.data_ptr(), moves.data_ptr(), counts.data_ptr())
    eng.chess_children_async(n, st.data_ptr(), kids.data_ptr(), kmoves.data_ptr(), kcounts.data_ptr())
    eng.chess_children_async(n, st.data_ptr(), kids2.data_ptr(), 0, k2counts.data_ptr())
    eng.debug_chess_probe_async(n, st.data_ptr(), probe.data_ptr())
    eng.chess_terminal_async(n, st.data_ptr(), flags.data_ptr())
    torch.cuda.synchronize()
    moves, kmoves = moves.cpu().numpy().view(np.uint16), kmoves.cpu().numpy().view(np.uint16)
    counts, kcounts, k2counts = counts.cpu().numpy(), kcounts.cpu().numpy(), k2counts.cpu().numpy()
    assert torch.equal(kids, kids2)
    kids = kids.cpu().numpy().reshape(n, MAXM, 72)
    probe, flags = probe.cpu().numpy(), flags.cpu().numpy()
    for i, (name, s) in enumerate(pos):
        if want_n[i] > MAXM:
            assert counts[i] == kcounts[i] == k2counts[i] == -1, (i, name)
            assert (moves[i] == FILL).all() and (kmoves[i] == FILL).all() and (kids[i] == 0xA5).all(), (i, name)
            assert probe[i] in (-1, -2) and flags[i] == 8, (i, name, probe[i], flags[i])
            if "no king" in name:   # no bit view: the probe generates the list
                assert probe[i] == -1, (i, name)
            continue
        want = oracle.chess_moves(s)
        k = len(want)
        assert counts[i] == kcounts[i] == k2counts[i] == k, (i, name)
        assert [decode(m) for m in moves[i, :k]] == [list(m) for m in want], (i, name)
        assert (moves[i, :k] == kmoves[i, :k]).all(), (i, name)
        assert (moves[i, k:] == FILL).all() and (kmoves[i, k:] == FILL).all() and (kids[i, k:] == 0xA5).all(), (i, name)
        assert probe[i] in (-2, k) and (k > 0 or probe[i] == 0), (i, name, probe[i])
        assert flags[i] == 0, (i, name, flags[i])   # every position here has a move and a young fifty counter
        for j, m in enumerate(want):
            o = oracle.chess_play(s, m)
            assert bytes(kids[i, j, :64]) == bytes(o.board), (i, name, j)
            assert kids[i, j, 64:67].tolist() == [o.turn, o.fifty, o.castle] and not kids[i, j, 67:].any(), (i, name, j)


def test_crowded_boards_match_oracle(eng):
    """The generator's fallback above 128 runs on crowded boards (and the run-parallel
    generator on their thinned-out twins): move lists vs the oracle."""
    import oracle
    from zeroclone_amd._native import CHESS_STATE_DTYPE
    pos, stats = _dense_boards()
    assert sum(r > 128 for r, _ in stats) >= 100 and sum(r <= 128 for r, _ in stats) >= 100
    for b, _, _ in CAPACITY_BOARDS.values():   # and the boards at and above 256 legal moves
        pos.append((b.encode("latin-1"), 0, 0, 0))
        stats.append(_count_runs(list(b), 0))
    assert max(m for _, m in stats) <= 512
    a = np.zeros(len(pos), CHESS_STATE_DTYPE)
    for i, (b, t, f, c) in enumerate(pos):
        a[i]["board"] = np.frombuffer(b, np.uint8)
        a[i]["turn"], a[i]["fifty"], a[i]["castle"] = t, f, c
    moves, counts = legal(eng, dev(a))
    over = 0
    for i, (b, t, fifty, c) in enumerate(pos):
        s = oracle.chess_state(b.decode("latin-1"), t, fifty, c)
        if oracle.chess_move_count(s) > MAXM:
            assert counts[i] == -1, (i, b)
            over += 1
            continue
        want = [list(m) for m in oracle.chess_moves(s)]
        assert counts[i] == len(want), (i, b, stats[i])
        assert [decode(m) for m in moves[i, :counts[i]]] == want, (i, b, stats[i])
    assert over == 4


PROBE_FENS = [
    "rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3",   # checkmated
    "k7/8/1Q6/8/8/8/8/7K b - - 0 1",                                   # stalemate
    "4k3/8/8/8/8/8/4r3/4K3 w - - 0 1",                                 # in check, king moves
    "4k3/4r3/8/8/8/8/4B3/4K3 w - - 0 1",                               # the bishop pinned on the king's file
    "7k/8/8/8/8/2b5/1P6/K7 w - - 0 1",                                 # pawn pinned on the king's diagonal
    "4k3/8/8/8/8/8/8/r3K2r w - - 0 1",                                 # king boxed on its rank
    "8/8/8/8/8/5k2/6q1/7K w - - 0 1",                                  # checkmated in the corner
    "8/8/8/8/8/4k3/8/2r1K1r1 w - - 0 1",                               # checkmated on the back rank
    "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",
]


def test_lazy_node_probe_is_sound(eng):
    """The crude search's lazy-node probe (chess_device.h legal_moves_probe: the free-move test,
    then one pseudo-legal move per piece through the legality test, then the full generation),
    via zc_debug_chess_probe_async, against the oracle's get_legal_moves on every position of 150
    random playouts (checks, pins, captures, mates, stalemates) and crafted pins and mates: -2
    (a legal move proven, no list) only where the list is non-empty, the exact length elsewhere."""
    import random

    import oracle
    from zeroclone_amd._native import CHESS_STATE_DTYPE
    rng = random.Random(11)
    states = [oracle.chess_from_fen(f) for f in PROBE_FENS]
    for _ in range(150):
        s = oracle.chess_init()
        for _ in range(160):
            states.append(s)
            ms = oracle.chess_moves(s)
            if not ms:
                break
            s = oracle.chess_play(s, rng.choice(ms))
    a = np.zeros(len(states), CHESS_STATE_DTYPE)
    for i, s in enumerate(states):
        a[i]["board"] = np.frombuffer(bytes(s.board), np.uint8)
        a[i]["turn"], a[i]["fifty"], a[i]["castle"] = s.turn, s.fifty, s.castle
    out = torch.zeros(len(states), dtype=torch.int32, device="cuda")
    eng.debug_chess_probe_async(len(states), dev(a).data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = np.array([len(oracle.chess_moves(s)) for s in states])
    lazy = got == -2
    assert np.all(want[lazy] > 0), np.flatnonzero(lazy & (want == 0))[:10]
    np.testing.assert_array_equal(got[~lazy], want[~lazy])
    assert lazy.mean() > 0.5 and (~lazy).sum() >= 20 and (want == 0).sum() >= 5
