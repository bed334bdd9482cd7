"""A book of openings, the host side: the pools' and the arenas' refusals (raised before an engine
exists, so no GPU is needed), the Connect4 book check, tests/traj_openings_ref.py's model of
zc_traj_openings_async against hand-written cases, and `openings_from_games` against a plain loop."""
import pytest
import torch

import traj_ref as tr
from traj_openings_ref import OpeningsModel, opening_of
from zeroclone_amd import selfplay
from zeroclone_amd.arena import C4Arena, ChessArena
from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay, TrajBatch, check_c4_book, openings_from_games


def c4_row(cols: str) -> list[int]:
    """The Connect4 row after the moves `cols` (digits: columns) from the empty board."""
    stones, height = [0, 0], [0] * 7
    for i, ch in enumerate(cols):
        c = int(ch)
        stones[i & 1] |= 1 << (7 * c + height[c])
        height[c] += 1
    return [stones[0], stones[1], len(cols) & 1]


BOOK = torch.tensor([c4_row("33"), c4_row("3"), c4_row("3342")], dtype=torch.int64)   # one at an odd ply
FENS = ["8/8/4k3/8/8/8/3QK3/8 w - - 96 60", "8/8/4k3/8/8/8/3QK3/8 b - - 97 60"]


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [torch.zeros((2, 4), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int32),
                                 torch.zeros(3, dtype=torch.int64), torch.zeros((0, 3), dtype=torch.int64),
                                 [[0, 0, 0]], "33"], ids=["width", "dtype", "rank", "empty", "list", "str"])
def test_c4_pool_refuses_a_malformed_book(bad):
    with pytest.raises(ValueError, match="openings"):
        C4SelfPlay(8, 32, openings=bad)


@pytest.mark.parametrize("bad", [torch.zeros((2, 72), dtype=torch.int64), torch.zeros((2, 9), dtype=torch.uint8),
                                 torch.zeros((0, 72), dtype=torch.uint8), [], [FENS[0], 3], BOOK],
                         ids=["dtype", "width", "empty", "no-fens", "not-a-fen", "c4-book"])
def test_chess_pool_refuses_a_malformed_book(bad):
    with pytest.raises(ValueError, match="openings"):
        ChessSelfPlay(4, 16, openings=bad)


def test_pools_refuse_a_book_without_the_recorder_or_with_the_fused_policy():
    with pytest.raises(ValueError, match="record=True"):
        C4SelfPlay(8, 32, openings=BOOK, record=False)
    with pytest.raises(ValueError, match="fused"):
        C4SelfPlay(8, 32, openings=BOOK, record_policy=True, fused_policy=True)
    with pytest.raises(ValueError, match="fused"):
        ChessSelfPlay(4, 16, openings=FENS, record_policy=True, fused_policy=True)


@pytest.mark.parametrize("arena,book", [(C4Arena, BOOK[:, :2]), (ChessArena, [])], ids=["c4", "chess"])
def test_arenas_refuse_a_malformed_book(arena, book):
    with pytest.raises(ValueError, match="openings"):
        arena(8, 20, batch_size=8, net_a=object(), net_b=object(), openings=book)


@pytest.mark.parametrize("cls", [C4SelfPlay, ChessSelfPlay])
def test_the_fused_launches_refuse_a_pool_with_a_book(cls):
    """run(), run_pooled() and drain() refuse first thing, before they touch any state: a pool
    that was never constructed shows it without an engine."""
    pool = object.__new__(cls)
    pool.book, pool.results = BOOK, torch.zeros(1)
    with pytest.raises(ValueError, match="book of openings"):
        pool.run(4)
    with pytest.raises(ValueError, match="book of openings"):
        pool.run_pooled(64, 4)
    if cls is C4SelfPlay:
        with pytest.raises(ValueError, match="book of openings"):
            pool.drain()


def test_the_shares():
    assert C4SelfPlay._openings_share == ChessSelfPlay._openings_share == 1
    assert C4Arena._openings_share == ChessArena._openings_share == 2


def _bare_arena(puct: bool, conv_head: bool = False):
    a = object.__new__(C4Arena)
    a.ps, a.vs, a._conv_head, a.dev = (object() if puct else None), (None if puct else object()), conv_head, "cpu"
    return a


def test_set_networks_refuses_another_search_or_head():
    from zeroclone_amd.nets import PolicyValueNetwork, ValueNetwork
    value = ValueNetwork(8, 1, in_planes=2)
    lin = PolicyValueNetwork(in_planes=2, board=(6, 7), n_logits=7)
    conv = PolicyValueNetwork(in_planes=17, board=(8, 8), n_logits=4096, head="conv")
    with pytest.raises(ValueError, match="value search"):
        _bare_arena(False)._inference_pair(value, lin)
    with pytest.raises(ValueError, match="PUCT search"):
        _bare_arena(True)._inference_pair(value, value)
    with pytest.raises(ValueError, match="conv_head"):
        _bare_arena(True, conv_head=False)._inference_pair(lin, conv)
    with pytest.raises(ValueError, match="conv_head"):
        _bare_arena(True, conv_head=True)._inference_pair(lin, lin)
    with pytest.raises(ValueError, match="set_networks"):
        _bare_arena(False).set_network(value)


# ------------------------------------------------------------------ the Connect4 book check
def test_the_book_check_passes_positions_games_reach():
    check_c4_book(BOOK)
    check_c4_book(torch.tensor([c4_row(""), c4_row("0123456"), c4_row("333333"), c4_row("0" * 6 + "1" * 6 + "2" * 5)]))


FULL = "".join(str(c) * 6 for c in (0, 1, 2, 4, 5, 6, 3))   # 42 stones; whether a line formed is not the point


@pytest.mark.parametrize("row,why", [
    ([1, 1, 0], "overlapping"),
    ([1 << 6, 0, 1], "sentinel"),
    ([1 << 49, 0, 1], "sentinel"),
    ([-1, 0, 1], "sentinel"),
    ([1 << 1, 0, 1], "gap"),
    ([1 << 7 | 1 << 9, 1 << 8 | 1, 0], None),                        # a column of four stones, no gap: fine
    ([1 | 1 << 2, 1 << 7, 1], "gap"),
    (c4_row("3")[:2] + [0], "turn"),
    (c4_row("33")[:2] + [1], "turn"),
    ([1 | 1 << 7, 0, 2], "turn"),
    ([0, 1, -1], "turn"),
    (c4_row("33")[:2] + [1 << 32], "turn"),
    (c4_row("0101010"), "four in a row"),                            # vertical, the side with turn 0
    (c4_row("0011223"), "four in a row"),                            # horizontal
    (c4_row("61516151"), "four in a row"),                           # vertical, the other side (column 1)
    (c4_row("01123223633"), "four in a row"),                        # a rising diagonal, columns 0 .. 3
    (c4_row("65543443033"), "four in a row"),                        # a falling diagonal, columns 6 .. 3
    (c4_row(FULL), "four in a row|full"),
])
def test_the_book_check_names_the_first_bad_row(row, why):
    book = torch.cat([BOOK, torch.tensor([row], dtype=torch.int64), torch.tensor([[1, 1, 0]])])
    if why is None:
        with pytest.raises(ValueError, match=r"row 4: overlapping"):
            check_c4_book(book)
        return
    with pytest.raises(ValueError, match=rf"row 3: .*({why})"):
        check_c4_book(book)


def test_the_book_check_refuses_a_full_board_without_a_line():
    """21 stones each, every column full, no four in a row on either side: only "full" is wrong."""
    s0, s1 = 0x3118E64D5B0C, 0xCCE311A284B3
    assert s0 & s1 == 0 and s0 | s1 == sum(0x3F << (7 * c) for c in range(7))
    with pytest.raises(ValueError, match="row 0: a full board"):
        check_c4_book(torch.tensor([[s0, s1, 0]], dtype=torch.int64))


# ------------------------------------------------------------------ the model, by hand
def book_rows(n: int, words: int) -> list[tuple]:
    return [tuple(0x2222000000000000 + (r + 1) * 0x100 + w for w in range(words)) for r in range(n)]


def run_model(n, lengths, steps, book, share, quota, words=3):
    t = tr.scripted(n, steps, 8 * words, lengths)
    m = OpeningsModel(n, tr.init_row(words), 8, 400, 100, quota, book=book, share=share)
    roots = m.seed(m.start_roots())
    seen = [list(roots)]
    for k in range(steps):
        states = [tuple(int(x) for x in r) for r in t["states"][k]]
        m.step_seeded(states, t["moves"][k], [int(x) for x in t["results"][k]], roots)
        seen.append(list(roots))
    return m, seen, t


def test_model_share_1_three_rows():
    """Three slots, no quota.  Slots 0 and 2 finish at step 0 (games 3, 4), slot 1 at step 1
    (game 5), slots 0 and 2 again at step 2 (games 6, 7)."""
    B, I = book_rows(3, 3), tr.init_row(3)
    m, seen, t = run_model(3, [[2, 3, 9], [3, 9], [2, 3, 9]], 3, B, 1, None)
    assert seen[0] == [B[0], B[1], B[2]]
    assert seen[1] == [B[0], tr.row_of(1, 0, 1, 3), B[1]]               # games 3 and 4
    assert seen[2] == [tr.row_of(0, 1, 1, 3), B[2], tr.row_of(2, 1, 1, 3)]   # game 5
    assert seen[3] == [B[0], tr.row_of(1, 1, 1, 3), B[1]]               # games 6 and 7
    assert [s[1] for s in m.slot] == [6, 5, 7] and I not in seen[3]
    firsts = {rec[0]: m.pool[rec[3]] for rec in m.games if rec}
    assert firsts == {0: B[0], 1: B[1], 2: B[2], 3: B[0], 4: B[1]}
    assert m.hist[0][0] == B[0] and m.hist[1][0] == B[2] and m.hist[2][0] == B[1]


def test_model_share_2_pairs_the_games():
    B = book_rows(3, 3)
    m, seen, _ = run_model(4, [[2] * 9] * 4, 3, B, 2, None)
    assert seen[0] == [B[0], B[0], B[1], B[1]]                          # games 0 .. 3
    assert seen[1] == [B[2], B[2], B[0], B[0]]                          # games 4 .. 7: 2, 2, 3 % 3, 3 % 3
    assert seen[2] == [B[1], B[1], B[2], B[2]]                          # games 8 .. 11
    assert all(m.pool[rec[3]] == B[opening_of(rec[0], 3, 2)] for rec in m.games if rec) and m.n_games == 12


@pytest.mark.parametrize("share", [1, 2])
def test_model_one_row(share):
    B = book_rows(1, 9)
    m, seen, _ = run_model(3, [[2, 3, 2, 2]] * 3, 4, B, share, None, words=9)
    assert seen[0] == [B[0]] * 3 and all(m.pool[rec[3]] == B[0] for rec in m.games if rec) and m.n_games >= 6


def test_model_quota_below_the_slot_count():
    """Quota 3 on five slots: slots 3 and 4 idle at d_init from the start, and a finished slot
    goes idle at d_init (no game left to start)."""
    B, I = book_rows(3, 3), tr.init_row(3)
    m, seen, _ = run_model(5, [[2, 2], [3, 2], [4, 2], [2], [2]], 3, B, 1, 3)
    assert seen[0] == [B[0], B[1], B[2], I, I]
    assert seen[1] == [I, tr.row_of(1, 0, 1, 3), tr.row_of(2, 0, 1, 3), I, I]
    assert seen[3] == [I] * 5 and m.finished == 3 and all(s == [1, -1] for s in m.slot)
    assert [m.pool[rec[3]] for rec in sorted(r for r in m.games if r)] == B


def test_model_quota_runs_out_inside_a_step():
    """Quota 6 on five slots: all five finish at step 0, slot 0 takes game 5 (opening 5 % 3 with
    share 1), the others go idle."""
    B, I = book_rows(3, 3), tr.init_row(3)
    m, seen, _ = run_model(5, [[2, 2]] * 5, 2, B, 1, 6)
    assert seen[0] == [B[0], B[1], B[2], B[0], B[1]]
    assert seen[1] == [B[2], I, I, I, I]
    assert seen[2] == [I] * 5 and m.finished == 6
    assert {rec[0]: m.pool[rec[3]] for rec in m.games if rec} == {g: B[g % 3] for g in range(6)}


@pytest.mark.parametrize("share", [1, 2])
def test_model_a_book_larger_than_the_quota(share):
    B = book_rows(8, 3)
    m, seen, _ = run_model(3, [[2, 2, 2]] * 3, 3, B, share, 5)
    assert m.finished == 5
    assert {rec[0]: m.pool[rec[3]] for rec in m.games if rec} == {g: B[g // share] for g in range(5)}
    assert set(B[5 // share + 1:]).isdisjoint(x for s in seen for x in s)   # the rows beyond are never used


def test_model_seed_is_idempotent_and_leaves_games_in_progress():
    B = book_rows(3, 3)
    m, seen, _ = run_model(3, [[2, 3, 9], [3, 9], [2, 3, 9]], 2, B, 1, None)
    before = ([list(h) for h in m.hist], list(seen[-1]))
    roots = m.seed(list(seen[-1]))
    assert ([list(h) for h in m.hist], roots) == before
    with pytest.raises(ValueError):
        OpeningsModel(3, tr.init_row(3), 8, 10, 10, book=[], share=1)
    with pytest.raises(ValueError):
        OpeningsModel(3, tr.init_row(3), 8, 10, 10, book=B, share=0)


# ------------------------------------------------------------------ openings_from_games
def make_batch(lengths, words, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows, games = [], []
    for no, ln in enumerate(lengths):
        games.append([no, no % 4, 0, len(rows), ln])
        for i in range(ln):
            # few distinct values, so that games share positions; negative words too
            rows.append(torch.randint(-2, 2, (words,), generator=g).tolist() if i else [0] * words)
    rows = torch.tensor(rows, dtype=torch.int64).reshape(-1, words)
    n = rows.shape[0]
    return TrajBatch(rows, torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int16),
                     torch.tensor(games, dtype=torch.int64).reshape(-1, 5))


def plain_loop(batch, ply, limit):
    seen = set()
    for _, _, _, first, ln in batch.games.tolist():
        if ln > ply + 1:
            seen.add(tuple(batch.rows[first + ply].tolist()))
    out = sorted(seen)          # torch.unique(dim=0): rows in lexicographic order of their words
    return out if limit is None else out[:limit]


@pytest.mark.parametrize("words", [3, 9])
@pytest.mark.parametrize("ply", [0, 1, 2, 5])
def test_openings_from_games_is_the_plain_loop(words, ply):
    batch = make_batch([2, 3, 4, 7, 3, 9, 2, 6, 4, 4, 8, 3] * 3, words, seed=ply)
    for limit in (None, 0, 1, 3, 1000):
        got = openings_from_games(batch, ply, limit)
        want = plain_loop(batch, ply, limit)
        if words == 9:
            assert got.dtype == torch.uint8 and got.shape[1:] == (72,)
            got = got.view(torch.int64)
        assert got.dtype == torch.int64 and got.tolist() == [list(r) for r in want]
    n_long = sum(1 for ln in batch.games[:, 4].tolist() if ln > ply + 1)
    full = openings_from_games(batch, ply)
    assert full.shape[0] <= n_long and (ply == 0) == (full.shape[0] == 1)      # duplicates collapse
    assert torch.equal(openings_from_games(batch, ply, 2), full[:2])           # a stable prefix


def test_openings_from_games_skips_short_games_and_takes_no_last_position():
    batch = make_batch([2, 2, 3], 3)
    assert openings_from_games(batch, 2).shape == (0, 3)          # no game has more than 3 positions
    one = openings_from_games(batch, 1)                            # the 3-position game alone
    assert one.tolist() == [batch.rows[int(batch.games[2, 3]) + 1].tolist()]
    with pytest.raises(ValueError):
        openings_from_games(batch, -1)
    assert selfplay.openings_from_games is openings_from_games
