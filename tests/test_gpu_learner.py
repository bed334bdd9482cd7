"""The learner on the device: zc_train_batch_async and zc_train_loss_async against their
executable spec (tests/learner_ref.py) and the entry points they must agree with, the autograd
wrapper, and one training run handed back to a running pool.  The smallest shapes that cross
the kernels' boundaries: one row, a partial workgroup (5 = 4 + 1 rows), more than one workgroup
with a partial one (66, 67), a chess row with more than 64 legal moves (a lane holds two) and
one with none; and the sizes training reaches: rows with up to 218 entries and 256 legal moves
(four to a lane), more rows than the reduction has threads, other strides, the rows the header
rules on but no minibatch holds, the C entry points' own refusals and a captured graph."""
import ctypes

import numpy as np
import pytest
import torch

import learner_ref
from conftest import load_golden
from zeroclone_amd import _native, learner
from zeroclone_amd.learner import TrainingSet
from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay, TrajBatch, dataset_labels, planes, simulate_games

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIFTY_SOON = "4k3/8/8/8/8/8/8/4K2R w K - 46 30"   # the fifty-move rule ends a game within four plies
MANY_MOVES, MATED = 171, 115                       # chess_movelists.json: 65 legal moves; none, in check


def _np(ts):
    f = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return f(ts.rows), f(ts.labels), f(ts.pi_off), f(ts.pi)


def _empty_csr(n):
    return torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)


def _dense(ts, width):
    """TrajBatch.policy_targets of the whole set (zc_traj_policy_dense_async)."""
    return TrajBatch(ts.rows, ts.labels, None, None, ts.pi_off, ts.pi).policy_targets(width)


# ---------------------------------------------------------------- the batch, Connect4
@pytest.fixture(scope="module")
def c4_set():
    """The c4_selfplay.json games (no visit counts) and one pool's games with theirs."""
    rows, labels = [], []
    for g in load_golden("c4_selfplay.json")["games"]:
        s, turn, height = [0, 0], 0, [0] * 7
        states = [(0, 0, 0)]
        for col in g["moves"]:
            s[turn] |= 1 << (7 * col + height[col])
            height[col] += 1
            turn ^= 1
            states.append((s[0], s[1], turn))
        rows += states
        labels.append(dataset_labels(len(states), g["result"]))
    fix = TrainingSet("c4", torch.tensor(rows, dtype=torch.int64),
                      torch.from_numpy(np.concatenate(labels).astype(np.int32)), *_empty_csr(len(rows)))
    pool = C4SelfPlay(games=8, sims=32, record_policy=True)
    simulate_games(pool, 8)
    batch = pool.last_batch
    pool.close()
    ts = TrainingSet.cat([fix.to(DEV), TrainingSet.from_batch(batch, "c4")])
    last = (len(fix) + batch.games[:, 3] + batch.games[:, 4] - 1).cpu().tolist()   # each pool game's last row
    return ts, last, _dense(ts, 7)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("B", [5, 67])
def test_c4_batch(c4_set, B, f16):
    ts, last, dense = c4_set
    n = len(ts)
    rows = ts.rows.cpu().numpy()
    occ = rows[:, 0] | rows[:, 1]
    full = [i for i in range(n) if any((int(occ[i]) >> (7 * c + 5)) & 1 for c in range(7))]
    with_pi = (ts.pi_off[1:] > ts.pi_off[:-1]).nonzero().reshape(-1).cpu().tolist()
    assert full and with_pi
    idx = [(n - 1 - 29 * k) % n for k in range(B)]                       # descending, wrapping round
    idx[:5] = [with_pi[-1], last[0], full[-1], with_pi[-1], with_pi[0]]   # a repeat, a game's end, a full column
    flags = np.asarray([k % 3 == 0 and k != 3 for k in range(B)], np.uint8)   # the repeat: once each way
    index = torch.tensor(idx, device=DEV)
    mb = learner.minibatch(ts, index, torch.from_numpy(flags).to(DEV), torch.float16 if f16 else torch.float32)
    mb.check()
    want = planes(rows[idx])
    want[flags == 1] = want[flags == 1][:, :, :, ::-1]
    assert mb.planes.dtype == (torch.float16 if f16 else torch.float32)
    np.testing.assert_array_equal(mb.planes.float().cpu().numpy(), want)
    np.testing.assert_array_equal(mb.z.cpu().numpy(), ts.labels[index].float().cpu().numpy())
    legal, nl, tgt = mb.legal.cpu().numpy(), mb.n_legal.cpu().numpy(), mb.target.cpu().numpy()
    d = dense[index].cpu().numpy()
    for b, i in enumerate(idx):
        cols = [c for c in range(7) if not (int(occ[i]) >> (7 * c + 5)) & 1]
        row = d[b]
        if flags[b]:
            cols, row = sorted(6 - c for c in cols), row[::-1]
        assert nl[b] == len(cols) and legal[b, :nl[b]].tolist() == cols and not legal[b, nl[b]:].any()
        np.testing.assert_array_equal(tgt[b, :nl[b]], row[cols])
        assert not tgt[b, nl[b]:].any()
        assert row.sum() == row[cols].sum()   # no visit count sits on a full column
    assert not tgt[1].any() and tgt[0].any() and nl[2] < 7
    ref = learner_ref.batch_ref("c4", *_np(ts), idx, flags)
    for k in ("planes", "z", "n_legal", "target"):
        np.testing.assert_array_equal(getattr(mb, k).float().cpu().numpy(), ref[k].astype(np.float32), err_msg=k)
    np.testing.assert_array_equal(legal.astype(np.uint16), ref["legal"])


def test_c4_batch_flags_a_bad_index_and_a_full_column(c4_set):
    ts, _, _ = c4_set
    n = len(ts)
    mb = learner.minibatch(ts, torch.tensor([0, n, -1, 1], device=DEV))
    assert int(mb.status.item()) == 2 and mb.n_legal.cpu().tolist() == [7, 0, 0, 7]
    assert not mb.planes[1:3].any() and not mb.target.any()
    with pytest.raises(RuntimeError, match="outside"):
        mb.check()
    rows = ts.rows[:2].clone()
    rows[1, 0] = 0x3F << 14   # column 2 full
    rows[1, 1] = 0
    bad = TrainingSet("c4", rows, ts.labels[:2], torch.tensor([0, 0, 2], device=DEV),
                      torch.tensor([2 | 5 << 16, 4 | 3 << 16], dtype=torch.int32, device=DEV))
    mb = learner.minibatch(bad, torch.tensor([1], device=DEV))
    assert int(mb.status.item()) == 1
    assert mb.legal[0].cpu().tolist() == [0, 1, 3, 4, 5, 6, 0]
    assert mb.target[0].cpu().tolist() == [0, 0, 0, float(np.float32(3) / np.float32(8)), 0, 0, 0]
    with pytest.raises(RuntimeError, match="not legal"):
        mb.check()


# ---------------------------------------------------------------- the batch, chess
@pytest.fixture(scope="module")
def chess_set():
    pool = ChessSelfPlay(games=4, sims=32, record_policy=True, init_fen=FIFTY_SOON, hist_cap=128)
    simulate_games(pool, 8, max_steps=400)
    batch = pool.last_batch
    cases = load_golden("chess_movelists.json")["cases"]
    hand = torch.from_numpy(np.stack([learner_ref.chess_row(cases[k]["state"]) for k in (MANY_MOVES, MATED, 0)]))
    assert len(cases[MANY_MOVES]["moves"]) > 64 and not cases[MATED]["moves"]
    extra = TrainingSet("chess", hand, torch.tensor([1, -1, 0], dtype=torch.int32), *_empty_csr(3)).to(DEV)
    ts = TrainingSet.cat([TrainingSet.from_batch(batch, "chess"), extra])
    yield ts, pool.eng, _dense(ts, 4096)
    pool.close()


def _chess_expected(eng, rows, f16):
    n = rows.shape[0]
    pl = torch.empty((n, 17, 8, 8), dtype=torch.float16 if f16 else torch.float32, device=DEV)
    mv = torch.zeros((n, 256), dtype=torch.int16, device=DEV)
    cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
    rows = rows.contiguous()
    eng.chess_planes_async(n, rows.data_ptr(), pl.data_ptr(), f16)
    eng.chess_legal_moves_async(n, rows.data_ptr(), mv.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    return pl, mv, cnt


def _chess_index(ts, B):
    n = len(ts)
    with_pi = (ts.pi_off[1:] > ts.pi_off[:-1]).nonzero().reshape(-1).cpu().tolist()
    idx = [(n - 1 - 5 * k) % n for k in range(B)]
    idx[:3] = [n - 3, n - 2, with_pi[-1]]   # more than 64 moves; mated; a searched position
    if B > 3:
        idx[3:6] = [with_pi[-1], with_pi[0], n - 3]
    return idx


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("B", [3, 66])
def test_chess_batch(chess_set, B, f16):
    ts, eng, dense = chess_set
    idx = _chess_index(ts, B)
    index = torch.tensor(idx, device=DEV)
    mb = learner.minibatch(ts, index, planes_dtype=torch.float16 if f16 else torch.float32)
    mb.check()
    pl, mv, cnt = _chess_expected(eng, ts.rows[index], f16)
    assert torch.equal(mb.planes, pl) and torch.equal(mb.legal, mv) and torch.equal(mb.n_legal, cnt)
    assert mb.n_legal[0] > 64 and mb.n_legal[1] == 0
    assert torch.equal(mb.z, ts.labels[index].float())
    live = torch.arange(256, device=DEV).view(1, -1) < cnt.view(-1, 1)
    want = dense[index].gather(1, learner.logit_index(mv, 4096)) * live
    assert torch.equal(mb.target, want)
    assert mb.target[2].sum() > 0.99 and not mb.target[:2].any()
    # every visit count sits on a legal move
    assert torch.allclose(want.sum(1), dense[index].sum(1), rtol=1e-6, atol=0)
    if B == 3 and not f16:   # the spec, through the chess oracle
        ref = learner_ref.batch_ref("chess", *_np(ts), idx)
        for k in ("planes", "z", "n_legal", "target"):
            np.testing.assert_array_equal(getattr(mb, k).cpu().numpy(), ref[k], err_msg=k)
        np.testing.assert_array_equal(mb.legal.cpu().numpy().view(np.uint16), ref["legal"])


def test_chess_batch_flags_an_illegal_entry_and_refuses_the_mirror(chess_set):
    ts, eng, _ = chess_set
    i = int((ts.pi_off[1:] - ts.pi_off[:-1]).argmax())
    lo, hi = int(ts.pi_off[i]), int(ts.pi_off[i + 1])
    assert hi - lo >= 2
    pi = ts.pi.clone()
    pi[lo] = (int(pi[lo]) >> 16) << 16   # from a8 to a8: no position's move
    bad = TrainingSet("chess", ts.rows, ts.labels, ts.pi_off, pi)
    index = torch.tensor([i, 0], device=DEV)
    mb = learner.minibatch(bad, index)
    assert int(mb.status.item()) == 1
    _, mv, cnt = _chess_expected(eng, ts.rows[index], False)
    live = torch.arange(256, device=DEV).view(1, -1) < cnt.view(-1, 1)
    want = _dense(bad, 4096)[index].gather(1, learner.logit_index(mv, 4096)) * live
    assert torch.equal(mb.target, want) and torch.equal(mb.legal, mv)
    assert 0 < float(mb.target[0].sum()) < 1   # the dropped entry's count stays in the sum
    with pytest.raises(RuntimeError, match="not legal"):
        mb.check()
    with pytest.raises(ValueError, match="mirror"):
        learner.minibatch(ts, index, torch.zeros(2, dtype=torch.bool, device=DEV))
    good = learner.minibatch(ts, index)
    c = _native.TrainSet()
    c.game, c.row_bytes, c.n_rows = _native.ZC_TRAIN_CHESS, 72, len(ts)
    c.d_rows, c.d_labels = ts.rows.data_ptr(), ts.labels.data_ptr()
    flags = torch.zeros(2, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _native.lib().zc_train_batch_async(ctypes.byref(c), 2, p(index), p(flags), _native.ZC_F32, p(good.planes),
                                            p(good.z), p(good.legal), p(good.n_legal), p(good.target), p(good.status),
                                            None)
    assert rc == _native.ZC_EINVAL


# ---------------------------------------------------------------- the batch at training sizes
# The widest roots of test_gpu_puct_noise.py, with visit counts on more moves than the 64 entries
# the chess kernel reads per trip of its entry loop (a root searched with 800 simulations has them).
WIDE_FENS = {218: "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1",
             194: "R6R/3Q4/1Q4Q1/4Q3/2Q5/5Q2/pp1Q4/kBNN1KB1 w - - 0 1",
             171: "R6R/3Q4/1Q4Q1/4Q3/8/5Q2/pp1Q4/kBNN1KB1 w - - 0 1",
             131: "R6R/3Q4/1Q6/8/8/5Q2/pp1Q4/kBNN1KB1 w - - 0 1",
             20: "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"}
BOARD_257 = "KQQQQQQQQ      Q       QQ      QQ      QQ  Q   QQ Q    QQQQQQQQk"   # test_gpu_chess.py CAPACITY_BOARDS
# set rows: 0-2 every legal move has an entry; 3, 4 the same position with 64 and 65 entries; 5 an
# entry that is no move at position 66 of 70; 6 more legal moves than a row holds; 7 a few entries;
# 8 none
WIDE_ROWS = [(218, None), (194, None), (171, None), (131, 64), (131, 65), (131, 70), (257, 0), (20, 9), (194, 0)]
BAD_ROW, OVER_ROW, BAD_AT = 5, 6, 66


@pytest.fixture(scope="module")
def wide_chess_set():
    """Hand-made chess rows with hand-made CSRs.  The entries of a row are its first `k` legal
    moves (all of them for k None) in a shuffled order, not the list's; the counts are drawn
    from a seeded generator, one of them 65535 and several 1."""
    import oracle
    g = np.random.default_rng(77)
    rows, off, pi = [], [0], []
    for r, (n, k) in enumerate(WIDE_ROWS):
        s = oracle.chess_state(BOARD_257) if n == 257 else oracle.chess_from_fen(WIDE_FENS[n])
        rows.append(learner_ref.chess_row(dict(board=bytes(s.board).decode("latin-1"), turn=s.turn, fifty=s.fifty,
                                               castle=s.castle)))
        assert oracle.chess_move_count(s) == n
        ids = [] if n == 257 else [_native.pack_chess_move(*m) for m in oracle.chess_moves(s)]
        ids = [ids[j] for j in g.permutation(len(ids) if k is None else k)] if ids else []
        if k is not None and r != BAD_ROW:
            assert len(ids) == k
        cnt = g.integers(2, 2000, len(ids))
        cnt[g.random(len(ids)) < 0.2] = 1
        if r == 0:
            cnt[100] = 65535
            assert ids[:8] != sorted(ids[:8]) and (cnt == 1).sum() >= 3
        if r == BAD_ROW:
            ids[BAD_AT] = 0        # from a8 to a8: no position's move
        pi += [(int(c) << 16) | int(i) for i, c in zip(ids, cnt)]
        off.append(len(pi))
    assert [b - a for a, b in zip(off, off[1:])] == [218, 194, 171, 64, 65, 70, 0, 9, 0]
    ts = TrainingSet("chess", torch.from_numpy(np.stack(rows)), torch.tensor([1, -1, 0, 1, 1, -1, 1, 0, -1], dtype=torch.int32),
                     torch.tensor(off, dtype=torch.int64), torch.from_numpy(np.asarray(pi, np.uint32).view(np.int32).copy()))
    return ts.to(DEV), ts


def _batch_is_the_spec(game, ts_dev, ts_cpu, idx, f16, flags=None):
    """minibatch bit for bit against learner_ref.batch_ref; returns (minibatch, the spec's)."""
    mb = learner.minibatch(ts_dev, torch.tensor(idx, device=DEV), None if flags is None else torch.tensor(flags, device=DEV),
                           torch.float16 if f16 else torch.float32)
    ref = learner_ref.batch_ref(game, *_np(ts_cpu), idx, flags)
    assert mb.planes.dtype == (torch.float16 if f16 else torch.float32)
    for k in ("planes", "z", "n_legal", "target"):
        np.testing.assert_array_equal(getattr(mb, k).float().cpu().numpy(), ref[k].astype(np.float32), err_msg=k)
    np.testing.assert_array_equal(mb.legal.cpu().numpy().view(np.uint16), ref["legal"])
    assert int(mb.status.item()) == ref["status"]
    return mb, ref


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("idx", [[0], [0, 7, 1, 3, 4], [4, 3, 2, 0, 0]])
def test_chess_batch_with_more_entries_than_one_trip_reads(wide_chess_set, idx, f16):
    """Rows whose entries take up to four trips of the 64-wide entry loop (218 entries), exactly
    one (64) and one more than one (65), B = 1 and B = 5."""
    mb, ref = _batch_is_the_spec("chess", *wide_chess_set, idx, f16)
    assert ref["status"] == 0
    mb.check()
    tgt = mb.target.cpu().numpy()
    for b, i in enumerate(idx):
        n, k = WIDE_ROWS[i]
        assert int(mb.n_legal[b]) == n and np.count_nonzero(tgt[b]) == (n if k is None else k)
        assert abs(float(tgt[b].astype(np.float64).sum()) - 1) < 1e-5 and not tgt[b, n:].any()
    if idx[0] == 0:   # the count of 65535 and the counts of 1 reached their moves
        cpu = wide_chess_set[1]
        cnt = (cpu.pi[:218].numpy().view(np.uint32) >> 16).astype(np.float32)
        assert tgt[0].max() == np.float32(65535) / cnt.sum() and tgt[0][tgt[0] > 0].min() == np.float32(1) / cnt.sum()


@pytest.mark.parametrize("f16", [False, True])
def test_chess_batch_drops_an_illegal_entry_of_the_second_trip(wide_chess_set, f16):
    """An entry that is no move, at position 66 of its row: only the second trip of the entry loop
    sees it.  Status 1, the entry dropped and its count still in the row's sum."""
    mb, ref = _batch_is_the_spec("chess", *wide_chess_set, [BAD_ROW, 7], f16)
    assert ref["status"] == 1
    cpu = wide_chess_set[1]
    lo = int(cpu.pi_off[BAD_ROW])
    cnt = (cpu.pi[lo:lo + 70].numpy().view(np.uint32) >> 16).astype(np.float64)
    got = mb.target[0].double().sum().item()
    assert np.count_nonzero(mb.target[0].cpu().numpy()) == 69
    assert abs(got - (1 - cnt[BAD_AT] / cnt.sum())) < 1e-6 and cnt[BAD_AT] / cnt.sum() > 1e-4
    assert abs(mb.target[1].double().sum().item() - 1) < 1e-6
    with pytest.raises(RuntimeError, match="not legal"):
        mb.check()


@pytest.mark.parametrize("f16", [False, True])
def test_chess_batch_refuses_a_position_with_257_legal_moves(wide_chess_set, f16):
    """Status bit 2: n_legal 0, the legal and target rows all zero, the planes and the label
    decoded all the same; the healthy rows beside it as the spec has them."""
    mb, ref = _batch_is_the_spec("chess", *wide_chess_set, [7, OVER_ROW, 0], f16)
    assert ref["status"] == 4 and mb.n_legal.cpu().tolist() == [20, 0, 218]
    assert not mb.legal[1].any() and not mb.target[1].any()
    assert float(mb.z[1]) == 1.0 and float(mb.planes[1].float().sum()) == sum(x != " " for x in BOARD_257) + 64   # the pieces, white to move
    assert np.count_nonzero(mb.target[0].cpu().numpy()) == 9 and np.count_nonzero(mb.target[2].cpu().numpy()) == 218
    with pytest.raises(RuntimeError, match=f"more than {_native.CHESS_MAX_MOVES} legal moves"):
        mb.check()


@pytest.fixture(scope="module")
def c4_long_rows():
    """Connect4 rows whose CSR holds more than 7 entries.  Row 0: column 2 full; entries with
    duplicate columns (the later one counts, a later count of 0 included) and ids 7 and 9 (no
    column: dropped, still in the sum).  Row 1: duplicates only.  Row 2: an empty board, no entry."""
    full2 = 0x15 << 14, 0x2A << 14
    rows = torch.tensor([[full2[0] | 1, full2[1] | 2, 0], [1 << 7, 1 << 21, 0], [0, 0, 0]], dtype=torch.int64)
    e = lambda col, cnt: col | cnt << 16   # noqa: E731
    pi = [e(0, 5), e(3, 7), e(0, 11), e(7, 4), e(6, 2), e(3, 9), e(9, 1), e(5, 3), e(6, 0),
          e(1, 4), e(1, 6), e(4, 1), e(0, 2), e(4, 8), e(6, 65535), e(2, 3), e(1, 1), e(0, 3)]
    ts = TrainingSet("c4", rows, torch.tensor([1, 0, -1], dtype=torch.int32), torch.tensor([0, 9, 18, 18]),
                     torch.from_numpy(np.asarray(pi, np.uint32).view(np.int32).copy()))
    return ts.to(DEV), ts


@pytest.mark.parametrize("f16", [False, True])
def test_c4_batch_with_more_than_seven_entries(c4_long_rows, f16):
    for idx, flags, status in (([1, 2, 1], [0, 1, 1], 0), ([0, 1, 2, 0], [0, 0, 0, 1], 1), ([0], [1], 1)):
        mb, ref = _batch_is_the_spec("c4", *c4_long_rows, idx, f16, np.asarray(flags, np.uint8))
        assert ref["status"] == status
    # by hand, the last call: row 0 mirrored.  Sum 42; columns 0, 3, 5 keep 11, 9, 3; column 6's later count is 0
    f = lambda k: float(np.float32(k) / np.float32(42))   # noqa: E731
    assert mb.legal[0].cpu().tolist() == [0, 1, 2, 3, 5, 6, 0] and int(mb.n_legal[0]) == 6
    assert mb.target[0].cpu().tolist() == [0, f(3), 0, f(9), 0, f(11), 0]


# ---------------------------------------------------------------- the loss
ULP1 = 4.8e-7   # 4 ulp of 1.0 in fp32


LANE_EDGES = (0, 63, 64, 127, 128, 191, 192, 255)   # lanes 0 and 63 of the four slots a lane holds


def _loss_case(width, B, f16, scale, policy=True, seed=0, counts=None, stride=None, most=None, policy_row=None):
    """Rows: 0 the longest legal list (70 moves: two to a lane / all 7 columns), 1 no legal move,
    every third a non-policy row, the last one with its legal logits near the dtype's largest
    finite value (the moves with a target all at one value, the others far below: the loss stays
    of order log n, and exp of an unshifted logit would overflow).
    counts: the rows' n_legal instead (distinct from/to pairs; a policy row then has a target on
    each of its moves LANE_EDGES); stride: the lists' stride; most: the longest list;
    policy_row(b): which rows have targets, instead of the rule above."""
    g = np.random.default_rng(1000 * width + 10 * B + seed)
    stride = stride or (7 if width == 7 else 256)
    most = most or min(stride, 7 if width == 7 else 70)
    legal = np.zeros((B, stride), np.uint16)
    target = np.zeros((B, stride), np.float32)
    if counts is None:
        nl = g.integers(1, most + 1, B)
        nl[0] = most
        if B > 1:
            nl[1] = 0
    else:
        nl = np.asarray(counts, np.int64)
        assert nl.shape == (B,) and nl.max() <= stride
    policy_row = policy_row or (lambda b: b % 3 != 2 or b == B - 1)
    logits = (g.standard_normal((B, width)) * scale).astype(np.float32)
    for b in range(B):
        n = int(nl[b])
        if width == 7:
            legal[b, :n] = np.sort(g.choice(7, n, replace=False))
        else:
            sq = g.choice(4096, n, replace=False)
            legal[b, :n] = (sq // 64) | ((sq % 64) << 6) | (g.integers(0, 10, n) << 12)
        if policy and n and policy_row(b):
            k = (g.integers(1, 33, n) * (g.random(n) < 0.7)).astype(np.int64)
            k[g.integers(0, n)] += 1
            if counts is not None:
                k[[j for j in LANE_EDGES if j < n]] += 1
            target[b, :n] = k.astype(np.float32) / np.float32(k.sum())
    b = B - 1
    if nl[b]:
        big = 6.0e4 if f16 else 3.0e38
        at = learner_ref.logit_index(legal[b, :nl[b]], width)
        logits[b, at] = np.where(target[b, :nl[b]] > 0, big, big * 0.9)
    v = np.tanh(g.standard_normal(B)).astype(np.float32)
    z = g.integers(-1, 2, B).astype(np.float32)
    return _case(width, f16, logits, v, z, legal, nl, target)


def _case(width, f16, logits, v, z, legal, nl, target):
    """The kernel's arguments on the device, and (np) what the spec reads: the logits as the
    kernel's dtype holds them."""
    B, stride = legal.shape
    lt = torch.from_numpy(np.asarray(logits, np.float32)).to(torch.float16 if f16 else torch.float32)
    v, z, target = np.asarray(v, np.float32), np.asarray(z, np.float32), np.asarray(target, np.float32)
    legal = np.ascontiguousarray(legal, np.uint16)
    return dict(B=B, width=width, stride=stride, logits=lt.to(DEV), v=torch.from_numpy(v).to(DEV),
                z=torch.from_numpy(z).to(DEV), legal=torch.from_numpy(legal.view(np.int16)).to(DEV),
                n_legal=torch.from_numpy(np.asarray(nl).astype(np.int32)).to(DEV), target=torch.from_numpy(target).to(DEV),
                np=dict(legal=legal, n_legal=nl, target=target, v=v, z=z, logits=lt.double().numpy()))


def _kernel(c, logits=True):
    """zc_train_loss_async straight: (loss [2], grad_v, grad_logits pre-filled with NaN)."""
    B = c["B"]
    need = _native.train_loss_scratch_bytes(B)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    loss = torch.full((2,), float("nan"), device=DEV)
    gv = torch.full((B,), float("nan"), device=DEV)
    gl = torch.full_like(c["logits"], float("nan"))
    lg = c["logits"] if logits else None
    _native.train_loss(B, c["width"], c["stride"], lg.data_ptr() if logits else 0, c["logits"].dtype == torch.float16,
                       c["v"].data_ptr(), c["z"].data_ptr(), c["legal"].data_ptr(), c["n_legal"].data_ptr(),
                       c["target"].data_ptr(), scratch.data_ptr(), need, loss.data_ptr(), gv.data_ptr(),
                       gl.data_ptr() if logits else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), gv.cpu().numpy(), gl.cpu()


def _mb(c):
    return learner.Minibatch(None, c["z"], c["legal"], c["n_legal"], c["target"], None, c["width"])


def _torch_fp32(c):
    """torch's own fp32 formulation (mse_loss, masked log_softmax, autograd) on the same inputs."""
    v = c["v"].clone().requires_grad_()
    x = c["logits"].float().clone().requires_grad_()
    Lv, Lp = learner.loss_torch(v, x, _mb(c))
    (Lv + Lp).backward()
    return Lv.item(), Lp.item(), v.grad.cpu().numpy(), x.grad.cpu().numpy()


def _check_loss(c, policy, label):
    """zc_train_loss_async on case c against the fp64 spec, with torch's fp32 formulation as the
    yardstick: every assertion of the loss tests."""
    width, B, f16 = c["width"], c["B"], c["logits"].dtype == torch.float16
    h = c["np"]
    Lv, Lp, gv, gl = learner_ref.loss_ref(h["v"], h["logits"], h["z"], h["legal"], h["n_legal"], h["target"])
    loss, kgv, kgl = _kernel(c)
    tLv, tLp, tgv, tgl = _torch_fp32(c)
    err = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - b)))   # noqa: E731
    figures = {"Lv": (err(loss[0], Lv), err(tLv, Lv)), "Lp": (err(loss[1], Lp), err(tLp, Lp)),
               "grad_v": (err(kgv, gv), err(tgv, gv))}
    if not f16:
        figures["grad_logits"] = (err(kgl.numpy(), gl), err(tgl, gl))
    print(f"{label} width {width} B {B} f16 {f16}: Lp {Lp:.6g}",
          {k: (f"{a:.3g}", f"{t:.3g}") for k, (a, t) in figures.items()})
    for k, (mine, torchs) in figures.items():
        assert mine <= 2 * torchs + ULP1, (label, k, mine, torchs)
    if f16:   # against the fp64 gradient rounded to fp16: within one fp16 ulp
        want = gl.astype(np.float16)
        got = kgl.numpy()
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(got)).astype(np.float16)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    # exact zeros off the policy rows' legal cells (the buffer held NaN)
    cells = np.zeros((B, width), bool)
    for b in range(B):
        n = min(max(int(h["n_legal"][b]), 0), c["stride"])
        at = learner_ref.logit_index(h["legal"][b, :n], width)
        if h["target"][b, :n][at < width].sum() > 0:
            cells[b, at[at < width]] = True
    got = kgl.float().numpy()
    assert not np.isnan(got).any() and not got[~cells].any()
    if not policy:
        assert loss[1] == 0.0 and not cells.any()
    else:
        assert cells.any() and np.isfinite(loss).all()
    # the same bits again
    loss2, kgv2, kgl2 = _kernel(c)
    assert loss.tobytes() == loss2.tobytes() and kgv.tobytes() == kgv2.tobytes()
    assert torch.equal(kgl.view(torch.int16 if f16 else torch.int32), kgl2.view(torch.int16 if f16 else torch.int32))
    # the value-only form
    vloss, vgv, vgl = _kernel(c, logits=False)
    assert vloss[0].tobytes() == loss[0].tobytes() and vloss[1] == 0.0 and vgv.tobytes() == kgv.tobytes()
    assert np.isnan(vgl.float().numpy()).all()   # untouched


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("width,B", [(7, 1), (7, 5), (7, 67), (4096, 3), (4096, 66)])
def test_loss_against_the_spec(width, B, f16):
    for scale, policy in ((1.0, True), (30.0, True), (1.0, False)):
        _check_loss(_loss_case(width, B, f16, scale, policy), policy, f"scale {scale} policy {policy}")


@pytest.mark.parametrize("f16", [False, True])
def test_loss_with_every_lane_slot_in_use(f16):
    """Width 4096 with 64 to 256 legal moves a row: a lane holds one to four of them, and the
    rows of 64, 128, 192 and 256 fill their last slot up to lane 63."""
    counts = [64, 65, 128, 129, 192, 193, 218, 256]
    for scale in (1.0, 30.0):
        c = _loss_case(4096, 8, f16, scale, counts=counts, policy_row=lambda b: b != 3)
        t = c["np"]["target"]
        assert all(t[b, j] > 0 for b, n in enumerate(counts) if b != 3 for j in LANE_EDGES if j < n)
        _check_loss(c, True, f"lane slots, scale {scale}")


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("width,B,late", [(7, 256, False), (7, 257, False), (7, 513, False), (7, 257, True),
                                          (7, 513, True), (4096, 513, False)])
def test_loss_with_more_rows_than_reduction_threads(width, B, late, f16):
    """B at and past the 256 threads of the reduction: a thread adds rows t, t + 256 and t + 512.
    With the default rows, thread 1 adds no policy row (row 1 has no legal move, row 257 no
    target), a thread with t % 3 == 0 two, the others one.  late: every policy row sits in the
    second pass or after (rows from 256 on)."""
    policy_row = (lambda b: b >= 256) if late else None
    c = _loss_case(width, B, f16, 1.0, policy_row=policy_row, most=None if width == 7 else 6)
    if not late and B > 257:
        pol = (c["np"]["target"].sum(1) > 0)
        per_thread = {int(pol[t::256].sum()) for t in range(256)}
        assert {0, 1, 2} <= per_thread and not pol[1::256][:2].any()
    _check_loss(c, True, f"rows, late {late}")


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("width,stride,B", [(7, 64, 9), (7, 1, 9), (4096, 218, 5), (4096, 1, 5)])
def test_loss_with_other_strides(width, stride, B, f16):
    counts = None
    if stride == 218:
        counts = [218, 0, 65, 1, 130]
    c = _loss_case(width, B, f16, 1.0, stride=stride, counts=counts)
    assert c["legal"].shape == (B, stride) and int(c["n_legal"].max()) == min(stride, 7 if width == 7 else 218)
    _check_loss(c, True, f"stride {stride}")


def test_loss_refuses_strides_out_of_range():
    c = _loss_case(7, 5, False, 1.0)
    for width, stride in ((7, 0), (7, 65), (7, 257), (4096, 0), (4096, 257), (7, -1)):
        c["width"], c["stride"] = width, stride
        with pytest.raises(ValueError, match="stride"):
            _kernel(c)


@pytest.mark.parametrize("f16", [False, True])
def test_loss_ignores_what_the_header_says_it_ignores(f16):
    """learner_ref.hand_made_rule_rows: ids 7, 63 and 0xFFFF in legal slots that carry a target,
    targets past n_legal or on an ignored id only, n_legal -3 and stride + 5."""
    h = learner_ref.hand_made_rule_rows()
    c = _case(7, f16, h["logits"], h["v"], h["z"], h["legal"], h["n_legal"], h["target"])
    gl = learner_ref.loss_ref(c["np"]["v"], c["np"]["logits"], c["np"]["z"], h["legal"], h["n_legal"], h["target"])[3]
    assert not gl[[3, 5, 6]].any() and gl[7].all() and gl[0, 6] != 0 and not gl[0, [0, 1, 3, 4]].any()
    _check_loss(c, True, "ignore rules")


def _poisoned(c, f16, legal_cell=None):
    """Case c with NaN, +inf and -inf in turn in every cell that is no legal move of its row; or
    with one NaN in the legal cell (row, slot)."""
    h = c["np"]
    logits = c["logits"].float().cpu().numpy().copy()
    if legal_cell is not None:
        b, j = legal_cell
        logits[b, learner_ref.logit_index(h["legal"][b, j:j + 1], c["width"])[0]] = np.nan
    else:
        k = 0
        for b in range(c["B"]):
            free = np.ones(c["width"], bool)
            free[learner_ref.logit_index(h["legal"][b, :int(h["n_legal"][b])], c["width"])] = False
            at = np.flatnonzero(free)
            logits[b, at] = np.asarray([np.nan, np.inf, -np.inf], np.float32)[(k + np.arange(len(at))) % 3]
            k += len(at)
        assert k > 0
    return _case(c["width"], f16, logits, h["v"], h["z"], h["legal"], h["n_legal"], h["target"])


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("width,B", [(7, 5), (4096, 3)])
def test_loss_reads_no_logit_but_the_legal_moves(width, B, f16):
    """Non-finite logits where no legal move points change no bit of any output; one NaN on a
    legal move of a policy row makes Lp non-finite and leaves Lv and grad_v alone."""
    c = _loss_case(width, B, f16, 1.0, seed=2)
    bits = lambda out: (out[0].tobytes(), out[1].tobytes(), out[2].view(torch.int16 if f16 else torch.int32))   # noqa: E731
    clean = bits(_kernel(c))
    got = bits(_kernel(_poisoned(c, f16)))
    assert got[0] == clean[0] and got[1] == clean[1] and torch.equal(got[2], clean[2])
    loss, gv, gl = _kernel(_poisoned(c, f16, legal_cell=(0, 0)))
    assert c["np"]["target"][0].sum() > 0 and not np.isfinite(loss[1])
    assert loss[:1].tobytes() == clean[0][:4] and gv.tobytes() == clean[1]
    assert not torch.isfinite(gl[0].float()).all() and torch.equal(gl[1:].view(clean[2].dtype), clean[2][1:])


@pytest.mark.parametrize("width,B,f16", [(7, 5, False), (4096, 3, True)])
def test_autograd_wrapper(width, B, f16):
    c = _loss_case(width, B, f16, 1.0, seed=1)
    loss, gv, gl = _kernel(c)
    grads = []
    for k in (1.0, 0.5):
        v = c["v"].clone().reshape(-1, 1).requires_grad_()
        x = c["logits"].clone().requires_grad_()
        Lv, Lp = learner.policy_value_loss(v, x, _mb(c))
        assert Lv.item() == loss[0] and Lp.item() == loss[1]
        ((Lv + Lp) * k).backward()
        grads.append((v.grad.reshape(-1).cpu().numpy(), x.grad.cpu()))
    assert grads[0][0].tobytes() == gv.tobytes() and torch.equal(grads[0][1], gl)
    assert (grads[1][0] == 0.5 * grads[0][0]).all() and torch.equal(grads[1][1], grads[0][1] * 0.5)
    v = c["v"].clone().requires_grad_()
    Lv, Lp = learner.policy_value_loss(v, None, _mb(c))
    Lv.backward()
    assert Lp.item() == 0.0 and v.grad.cpu().numpy().tobytes() == gv.tobytes()


# ---------------------------------------------------------------- end to end
def _small_net():
    from zeroclone_amd.nets import PolicyValueNetwork
    return PolicyValueNetwork(channels=8, blocks=1, in_planes=2, board=(6, 7), n_logits=7)


@pytest.fixture(scope="module")
def trained(c4_set):
    ts = c4_set[0].select(torch.arange(len(c4_set[0]) - 200, len(c4_set[0])))
    assert len(ts) == 200 and ts.pi.numel() > 0
    runs = []
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True   # the convolutions' backward without atomics
    try:
        for _ in range(2):
            torch.manual_seed(5)
            model = _small_net()
            g = torch.Generator().manual_seed(9)
            runs.append((model, learner.train(model, ts, epochs=3, lr=3e-3, batch_size=32, generator=g, mirror=True,
                                              device=DEV)))
    finally:
        torch.backends.cudnn.deterministic = was
    return runs


def test_training_lowers_the_loss_and_repeats(trained):
    (_, a), (_, b) = trained
    print("epoch losses", a.epoch_losses, "value", a.value_losses, "policy", a.policy_losses)
    assert len(a.epoch_losses) == 3 and a.epoch_losses[-1] < a.epoch_losses[0]
    assert a.policy_losses[0] > 0 and np.isfinite(a.reference_return)
    assert a.epoch_losses == b.epoch_losses and a.reference_return == b.reference_return


def test_set_network_hands_the_trained_weights_to_a_running_pool(trained):
    model = trained[0][0]
    torch.manual_seed(6)
    first = learner.inference_form(_small_net(), DEV)
    kw = dict(games=8, sims=16, seed=3, record_policy=True)
    pool = C4SelfPlay(puct_net=first, **kw)
    pool.step()
    fresh = C4SelfPlay(puct_net=learner.inference_form(model, DEV), **kw)
    fresh.adopt(pool)
    fresh.ps.search_no.copy_(pool.ps.search_no)   # the root noise is keyed by the search's number
    before = pool.ps.na.clone()
    pool.set_network(model)
    pool.step()
    fresh.step()
    torch.cuda.synchronize()
    pool.check()
    assert torch.equal(pool.ps.na, fresh.ps.na) and torch.equal(pool.moves, fresh.moves)
    assert int(pool.ps.na.sum()) > 0 and not torch.equal(pool.ps.na, before)
    assert torch.equal(pool.roots, fresh.roots)
    with pytest.raises(TypeError):
        pool.set_network(torch.nn.Linear(1, 1))
    plain = C4SelfPlay(games=2, sims=8)
    with pytest.raises(ValueError, match="without a network"):
        plain.set_network(model)
    for p in (pool, fresh, plain):
        p.close()


# ---------------------------------------------------------------- gradients through a model
def _param_grads(model, planes, mb, loss_fn):
    model.zero_grad()
    v, logits = model(planes)
    Lv, Lp = loss_fn(v, logits, mb)
    (Lv + Lp).backward()
    return float(Lv.detach()), float(Lp.detach()), {k: p.grad.detach().double().cpu().numpy() for k, p in model.named_parameters()}


@pytest.mark.parametrize("game", ["c4", "chess"])
def test_parameter_gradients_through_the_fused_loss(game, c4_set, wide_chess_set):
    """d(Lv + Lp)/d(parameters) of a small PolicyValueNetwork in training mode, three ways: the
    fused kernel, `loss_torch` in fp32 on the device, `loss_torch` on a float64 copy on the CPU
    (the reference).  Per tensor: the fused error at most twice torch-fp32's plus 4 ulp of the
    largest reference entry."""
    import copy
    from zeroclone_amd.nets import PolicyValueNetwork
    torch.manual_seed(11)
    if game == "c4":
        ts = c4_set[0]
        with_pi = (ts.pi_off[1:] > ts.pi_off[:-1]).nonzero().reshape(-1).cpu().tolist()
        without = (ts.pi_off[1:] == ts.pi_off[:-1]).nonzero().reshape(-1).cpu().tolist()
        idx = with_pi[:6] + without[:2] + with_pi[-5:]
        model = PolicyValueNetwork(channels=8, blocks=1, in_planes=2, board=(6, 7), n_logits=7)
    else:
        ts, idx = wide_chess_set[0], [0, 7, 8, 3, 4, 2]   # the 218-move row with its entries; row 8 has none
        model = PolicyValueNetwork(channels=8, blocks=1, in_planes=17, board=(8, 8), n_logits=4096)
    model = model.to(DEV).train()
    mb = learner.minibatch(ts, torch.tensor(idx, device=DEV))
    mb.check()
    assert (mb.target.sum(1) > 0).any() and (mb.target.sum(1) == 0).any()
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True   # the convolutions' backward without atomics
    try:
        fused = _param_grads(copy.deepcopy(model), mb.planes, mb, learner.policy_value_loss)
        torch32 = _param_grads(copy.deepcopy(model), mb.planes, mb, learner.loss_torch)
    finally:
        torch.backends.cudnn.deterministic = was
    cpu = learner.Minibatch(mb.planes.double().cpu(), mb.z.double().cpu(), mb.legal.cpu(), mb.n_legal.cpu(),
                            mb.target.double().cpu(), mb.status.cpu(), mb.width)
    ref = _param_grads(copy.deepcopy(model).cpu().double().train(), cpu.planes, cpu, learner.loss_torch)
    print(f"{game}: Lv {ref[0]:.6g} Lp {ref[1]:.6g}; fused {fused[0]:.6g} {fused[1]:.6g}; torch32 {torch32[0]:.6g} {torch32[1]:.6g}")
    assert ref[1] > 0
    for k, want in ref[2].items():
        mine, theirs = np.abs(fused[2][k] - want).max(), np.abs(torch32[2][k] - want).max()
        top = np.abs(want).max()
        print(f"  {k}: fused {mine:.3g} torch32 {theirs:.3g} max|ref| {top:.3g}")
        if top == 0:
            assert not fused[2][k].any(), k
        assert mine <= 2 * theirs + 4 * 2.0 ** -23 * top, (k, mine, theirs, top)


def test_train_reports_an_illegal_entry_of_any_batch_on_the_device():
    """test_learner_cpu.py's set on the device: the bad row is in the first of two batches, and
    `train` reads the OR of the epoch's status words."""
    from test_learner_cpu import _set_with_an_entry_on_a_full_column
    ts = _set_with_an_entry_on_a_full_column().to(DEV)
    assert int(learner.minibatch(ts, torch.arange(4)).status.item()) == 1
    assert int(learner.minibatch(ts, torch.arange(32, 64)).status.item()) == 0
    torch.manual_seed(3)
    with pytest.raises(RuntimeError, match="not legal"):
        learner.train(_small_net(), ts, epochs=1, lr=3e-3, batch_size=32, shuffle=False, device=DEV)
    res = learner.train(_small_net(), ts.select(torch.arange(1, 64)), epochs=1, lr=3e-3, batch_size=32, shuffle=False,
                        device=DEV)
    assert np.isfinite(res.epoch_losses).all()


# ---------------------------------------------------------------- the C entry points themselves
def _snapshot(outs):
    torch.cuda.synchronize()
    return [t.clone() for t in outs]


def _untouched(outs, before):
    torch.cuda.synchronize()
    return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, before))


def test_entry_points_refuse_bad_arguments(c4_long_rows):
    """zc_train_batch_async and zc_train_loss_async through ctypes, past the wrappers' own checks:
    each call breaks one documented condition, returns ZC_EINVAL and writes nothing."""
    L, P = _native.lib(), lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    ts = c4_long_rows[0]
    B = 3
    index = torch.tensor([0, 1, 2], device=DEV)
    flags = torch.zeros(B, dtype=torch.uint8, device=DEV)
    nan = float("nan")
    out = dict(planes=torch.full((B, 2, 6, 7), nan, device=DEV), z=torch.full((B,), nan, device=DEV),
               legal=torch.full((B, 7), 0x5A5A, dtype=torch.int16, device=DEV),
               n_legal=torch.full((B,), -7, dtype=torch.int32, device=DEV), target=torch.full((B, 7), nan, device=DEV),
               status=torch.zeros(1, dtype=torch.int32, device=DEV))
    before = _snapshot(out.values())

    def batch(B=B, dtype=_native.ZC_F32, null=None, use_set=True, flags=flags, **fields):
        c = _native.TrainSet()
        c.game, c.row_bytes, c.n_rows = _native.ZC_TRAIN_C4, 24, len(ts)
        c.d_rows, c.d_labels = ts.rows.data_ptr(), ts.labels.data_ptr()
        c.d_pi_off, c.d_pi = ts.pi_off.data_ptr(), ts.pi.data_ptr()
        for k, v in fields.items():
            setattr(c, k, v)
        a = dict(index=P(index), **{k: P(t) for k, t in out.items()})
        if null:
            a[null] = None
        return L.zc_train_batch_async(ctypes.byref(c) if use_set else None, B, a["index"], None if flags is None else P(flags),
                                      dtype, a["planes"], a["z"], a["legal"], a["n_legal"], a["target"], a["status"], None)

    bad = [dict(use_set=False), dict(B=-1), dict(dtype=2), dict(dtype=-1), dict(row_bytes=72), dict(row_bytes=0),
           dict(game=_native.ZC_TRAIN_CHESS), dict(game=2), dict(game=-1), dict(n_rows=-1), dict(d_pi=None), dict(d_pi_off=None),
           dict(d_rows=None), dict(d_labels=None), dict(game=_native.ZC_TRAIN_CHESS, row_bytes=72)]   # chess with flags
    bad += [dict(null=k) for k in ("index", "planes", "z", "legal", "n_legal", "target", "status")]
    for kw in bad:
        assert batch(**kw) == _native.ZC_EINVAL, kw
        assert _untouched(out.values(), before), kw
    assert batch(B=0) == _native.ZC_OK and _untouched(out.values(), before)
    assert batch() == _native.ZC_OK and batch(flags=None) == _native.ZC_OK   # the arguments were good but for the one
    torch.cuda.synchronize()
    assert int(out["status"].item()) == 1 and out["n_legal"].cpu().tolist() == [6, 7, 7]

    for width in (7, 4096):
        stride = 7 if width == 7 else 256
        c = _loss_case(width, B, False, 1.0)
        need = _native.train_loss_scratch_bytes(B)
        scratch = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
        o = dict(loss=torch.full((2,), nan, device=DEV), gv=torch.full((B,), nan, device=DEV),
                 gl=torch.full((B * width + 4,), nan, device=DEV))
        was = _snapshot(o.values())

        def loss(B=B, width=width, stride=stride, dtype=_native.ZC_F32, null=None, scratch_at=0, scratch_bytes=need,
                 grad_at=0):
            a = dict(logits=c["logits"].data_ptr(), v=c["v"].data_ptr(), z=c["z"].data_ptr(), legal=c["legal"].data_ptr(),
                     n_legal=c["n_legal"].data_ptr(), target=c["target"].data_ptr(), scratch=scratch.data_ptr() + scratch_at,
                     loss=o["loss"].data_ptr(), gv=o["gv"].data_ptr(), gl=o["gl"].data_ptr() + grad_at)
            if null:
                a[null] = None
            V = ctypes.c_void_p
            return L.zc_train_loss_async(B, width, stride, V(a["logits"]), dtype, V(a["v"]), V(a["z"]), V(a["legal"]),
                                         V(a["n_legal"]), V(a["target"]), V(a["scratch"]), scratch_bytes, V(a["loss"]),
                                         V(a["gv"]), V(a["gl"]), None)

        bad = [dict(B=0), dict(B=-1), dict(dtype=2), dict(width=8), dict(width=0), dict(stride=0), dict(stride=257),
               dict(stride=-1), dict(scratch_at=4), dict(scratch_bytes=need - 1), dict(scratch_bytes=0)]
        bad += [dict(null=k) for k in ("v", "z", "loss", "gv", "scratch", "legal", "n_legal", "target", "gl")]
        bad += [dict(stride=65)] if width == 7 else [dict(grad_at=4), dict(grad_at=8)]
        for kw in bad:
            assert loss(**kw) == _native.ZC_EINVAL, (width, kw)
            assert _untouched(o.values(), was), (width, kw)
        assert loss() == _native.ZC_OK and loss(scratch_at=16) == _native.ZC_OK
        if width == 7:   # no alignment asked of a 7-wide gradient
            assert loss(grad_at=4) == _native.ZC_OK
        assert loss(null="logits", width=8, stride=0, dtype=9) == _native.ZC_OK   # value only: the policy arguments are ignored
        torch.cuda.synchronize()
        assert torch.isfinite(o["loss"]).all()


def test_batch_and_loss_in_one_captured_graph(c4_set):
    """zc_train_batch_async then zc_train_loss_async captured on one stream (Connect4, B = 5) and
    replayed over new indices and logits: the eager calls' bits.  The status word is the caller's
    to zero: replays OR into it."""
    ts = c4_set[0]
    rows = ts.rows[:3].clone()
    rows[1, 0], rows[1, 1] = 0x3F << 14, 0   # column 2 full, with an entry on it
    bad = TrainingSet("c4", rows, ts.labels[:3].clone(), torch.tensor([0, 0, 2, 2], device=DEV),
                      torch.tensor([2 | 5 << 16, 4 | 3 << 16], dtype=torch.int32, device=DEV))
    ts = TrainingSet.cat([ts, bad])
    n, B = len(ts), 5
    with_pi = (ts.pi_off[1:] > ts.pi_off[:-1]).nonzero().reshape(-1).cpu().tolist()
    clean = [[with_pi[0], 3, with_pi[5], 0, with_pi[-2]], [with_pi[7], with_pi[2], 1, with_pi[9], with_pi[1]]]
    dirty = [with_pi[3], n - 2, with_pi[4], 2, with_pi[6]]
    g = torch.Generator().manual_seed(4)
    c = _native.TrainSet()
    c.game, c.row_bytes, c.n_rows = _native.ZC_TRAIN_C4, 24, n
    c.d_rows, c.d_labels, c.d_pi_off, c.d_pi = ts.rows.data_ptr(), ts.labels.data_ptr(), ts.pi_off.data_ptr(), ts.pi.data_ptr()
    need = _native.train_loss_scratch_bytes(B)

    def buffers():
        return dict(planes=torch.empty((B, 2, 6, 7), device=DEV), z=torch.empty(B, device=DEV),
                    legal=torch.empty((B, 7), dtype=torch.int16, device=DEV), n_legal=torch.empty(B, dtype=torch.int32, device=DEV),
                    target=torch.empty((B, 7), device=DEV), status=torch.zeros(1, dtype=torch.int32, device=DEV),
                    scratch=torch.empty(need, dtype=torch.uint8, device=DEV), loss=torch.empty(2, device=DEV),
                    gv=torch.empty(B, device=DEV), gl=torch.empty((B, 7), device=DEV))

    def enqueue(o, index, flags, logits, v):
        s = torch.cuda.current_stream().cuda_stream
        _native.train_batch(c, B, index.data_ptr(), flags.data_ptr(), False, o["planes"].data_ptr(), o["z"].data_ptr(),
                            o["legal"].data_ptr(), o["n_legal"].data_ptr(), o["target"].data_ptr(), o["status"].data_ptr(), s)
        _native.train_loss(B, 7, 7, logits.data_ptr(), False, v.data_ptr(), o["z"].data_ptr(), o["legal"].data_ptr(),
                           o["n_legal"].data_ptr(), o["target"].data_ptr(), o["scratch"].data_ptr(), need, o["loss"].data_ptr(),
                           o["gv"].data_ptr(), o["gl"].data_ptr(), s)

    index = torch.tensor(clean[0], device=DEV)
    flags = torch.tensor([0, 1, 0, 1, 1], dtype=torch.uint8, device=DEV)
    logits, v = torch.randn((B, 7), generator=g).to(DEV), torch.tanh(torch.randn(B, generator=g)).to(DEV)
    held = buffers()
    enqueue(buffers(), index, flags, logits, v)   # the kernels' code loaded before the capture
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        enqueue(held, index, flags, logits, v)
    held["status"].zero_()
    keys = ("planes", "z", "legal", "n_legal", "target", "loss", "gv", "gl")
    for idx, want_status, sticky in ((clean[0], 0, 0), (clean[1], 0, 0), (dirty, 1, 1), (clean[0], 0, 1)):
        index.copy_(torch.tensor(idx))
        logits.copy_(torch.randn((B, 7), generator=g))
        v.copy_(torch.tanh(torch.randn(B, generator=g)))
        flags.copy_(torch.randint(0, 2, (B,), generator=g).to(torch.uint8))
        graph.replay()
        eager = buffers()
        enqueue(eager, index, flags, logits, v)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(held[k].view(torch.uint8), eager[k].view(torch.uint8)), (k, idx)
        assert int(eager["status"].item()) == want_status and int(held["status"].item()) == sticky, idx
        assert torch.isfinite(held["loss"]).all() and float(held["loss"][1]) > 0
