"""The fused Connect4 search's MT19937 stream in LDS, generated in bulk (c4_device.h: LRng).

The kernel keeps a game's raw words in a 1024-word LDS ring and their 3-bit draws in a byte
ring beside it, positions relative to the launch's start rounded down to a multiple of 4, and
refills both 224 words at a time whenever fewer than 64 generated words lie ahead.  The parity
suites pin the common case; the cases here aim at what a bulk refill can get wrong: where the
stream starts (Engine.set_rng_state puts a game at any index 0..624 of a 624-word block, so
the starts below cover every alignment of the ring's origin, the seeded block's end at word
624, the first refill exactly at / one before / one after the first leaf's head, and — every
search here consumes more than 1024 words — the ring's wrap and several refill steps), the
hand-over to and from the HBM-ring kernels, carried moves, and the walk replay's skip.
The reference is always the oracle on the same MT state: move, root visit counts, and the
stream afterwards (all 624 state words and the index).
"""
import random

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

# index of the next word inside the block handed to set_rng_state (the block's words sit at the
# stream's positions 0..623, generated mark 624): the four origin alignments at the block's
# start; 397 = 624 - 227 (the recurrence's nearest input); 559 / 560 / 561: the first view has
# 65 / 64 / 63 generated words ahead; 562, 563: the other alignments there; 600: the first
# search's views straddle word 624; 621..624: the block's end, where everything is generated
STARTS = [0, 1, 2, 3, 337, 397, 559, 560, 561, 562, 563, 600, 621, 622, 623, 624]
G = len(STARTS)


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=G, max_sims=96, max_batch=32)
    yield e
    e.close()


def states(boards):
    from zeroclone_amd._native import C4_STATE_DTYPE, c4_from_rows
    out = np.zeros(len(boards), C4_STATE_DTYPE)
    for i, (b, t) in enumerate(boards):
        out[i] = c4_from_rows(b, t)
    return out


def mixed_boards(n, salt, max_plies=24):
    """n ongoing positions 0..max_plies plies into random games (a few of them the opening)."""
    rng = random.Random(salt)
    out = []
    while len(out) < n:
        b, t = "." * 42, 0
        ok = True
        for _ in range(rng.randint(0, max_plies) if len(out) % 4 else 0):
            b, t = oracle.play(b, t, rng.choice([c for c in range(7) if b[c] == "."]))
            if oracle.check_win(b, t) or oracle.check_draw(b):
                ok = False
                break
        if ok:
            out.append((b, t))
    return out


def mt_at(seed, index):
    """An oracle stream standing at `index` of a twisted block (one word drawn, then placed)."""
    mt = oracle.MT(seed)
    mt.u32()
    mt.s.index = index
    return mt


def put(eng, game, mt):
    words, index = mt.state()
    eng.set_rng_state(game, np.asarray(words, np.uint32), index)


def same_stream(eng, game, mt):
    got, gi = eng.get_rng_state(game)
    words, index = mt.state()
    return gi == index and np.array_equal(got, np.asarray(words, np.uint32))


def oracle_moves(boards, mts, sims, bs):
    out = []
    for (b, t), mt in zip(boards, mts):
        out.append(oracle.get_move_mt(b, t, mt, sims, 1.4, bs))
    return out


def check_search(mv, na, ref, tag):
    for i, (col, root_na, order) in enumerate(ref):
        assert int(mv[i]) == col, (tag, i)
        assert [int(na[i][c]) for c in order] == root_na, (tag, i)


@pytest.mark.parametrize("sims,bs", [(64, 8), (96, 32), (40, 32)])
def test_stream_position_sweep(eng, sims, bs):
    """Every start, one game each, against the oracle — none skipped."""
    boards = mixed_boards(G, 7 * sims + bs)
    mts = [mt_at(1000 + 17 * g + sims, s) for g, s in enumerate(STARTS)]
    for g, mt in enumerate(mts):
        put(eng, g, mt)
    before = [mt.drawn for mt in mts]
    mv, na, st = eng.c4_search(states(boards), sims, 1.4, bs)
    ref = oracle_moves(boards, mts, sims, bs)
    check_search(mv, na, ref, (sims, bs))
    words = [mt.drawn - b for mt, b in zip(mts, before)]
    assert [int(x) for x in st["rng_words"]] == words
    if sims >= 64:   # searches that wrap the ring (and take several refill steps) are among them
        assert sum(w > 1024 for w in words) >= G // 4
    for g, mt in enumerate(mts):
        assert same_stream(eng, g, mt), (sims, bs, STARTS[g])
    # a second search from where the first one left the stream (its own hand-over format)
    mv, na, st = eng.c4_search(states(boards), sims, 1.4, bs)
    check_search(mv, na, oracle_moves(boards, mts, sims, bs), (sims, bs, "again"))
    for g, mt in enumerate(mts):
        assert same_stream(eng, g, mt), (sims, bs, STARTS[g], "again")


def stepwise_search(eng, vs, boards, sims, bs):
    """zc_c4_ext_* on the games' HBM-ring streams, each flush's leaves rolled out on their game's
    stream in pending order (what Value('random_rollout') does in the reference)."""
    from zeroclone_amd._native import C4_STATE_DTYPE

    def value_fn(leaves, planes, counts):
        rows = leaves.cpu().numpy().copy()
        cnt = counts.cpu().numpy()
        per = rows.shape[0] // cnt.shape[0]
        rows[:, 2] &= 1
        out = np.zeros(rows.shape[0], np.float64)
        for g, k in enumerate(cnt):
            if k:
                st = np.ascontiguousarray(rows[g * per: g * per + k]).view(C4_STATE_DTYPE).reshape(k)
                out[g * per: g * per + k] = eng.c4_rollouts(st, game=g)[0]
        return torch.from_numpy(out).to(leaves.device)

    roots = torch.from_numpy(states(boards).view(np.int64).reshape(len(boards), 3).copy()).to(vs.dev)
    mv, na, st = vs.run(roots, sims, 1.4, value_fn)
    assert not st[:, 5].any()
    return mv.cpu().numpy(), na.cpu().numpy()


@pytest.mark.parametrize("bs", [8, 32])
def test_hand_over_both_ways(eng, bs):
    """Fused search (LDS stream), stepwise search (HBM ring), fused search again, each from the
    position the last move led to: three oracle searches in a row on the same stream."""
    from zeroclone_amd.valued import C4ValuedSearch
    n, sims = 8, 64
    starts = STARTS[4:12]
    boards = mixed_boards(n, 300 + bs, max_plies=16)
    mts = [mt_at(5000 + 31 * g + bs, s) for g, s in enumerate(starts)]
    for g, mt in enumerate(mts):
        put(eng, g, mt)
    vs = C4ValuedSearch(eng, n, bs, planes=False)
    for step in range(3):
        if step == 1:
            mv, na = stepwise_search(eng, vs, boards, sims, bs)
        else:
            mv, na, _ = eng.c4_search(states(boards), sims, 1.4, bs)
        check_search(mv, na, oracle_moves(boards, mts, sims, bs), (bs, step))
        for g, mt in enumerate(mts):
            assert same_stream(eng, g, mt), (bs, step, starts[g])
        nxt = []
        for g, (b, t) in enumerate(boards):  # play the move; a finished game goes on from the opening
            b2, t2 = oracle.play(b, t, int(mv[g]))
            nxt.append(("." * 42, 0) if oracle.check_win(b2, t2) or oracle.check_draw(b2) else (b2, t2))
        boards = nxt


@pytest.mark.parametrize("bs", [8, 32])
def test_carried_moves_resume_with_the_stream(bs):
    """Three carry launches whose budgets cut moves at different flushes, then drain(): every
    game's finished moves are its free-run moves, and its stream ends where the free run's
    stood after as many moves (tests/test_gpu_selfplay_run.py's carried-move case, small, on
    streams placed by set_rng_state)."""
    from zeroclone_amd.selfplay import C4SelfPlay
    n, sims, cap = 8, 64, 8
    budgets = [n * cap // 2, n * cap // 3, n * cap // 2]
    total = len(budgets) * cap + 1
    starts = STARTS[4:12]
    a = C4SelfPlay(n, sims, batch_size=bs, seed=13)
    b = C4SelfPlay(n, sims, batch_size=bs, seed=13)
    for sp in (a, b):
        for g, s in enumerate(starts):
            put(sp.eng, g, mt_at(9000 + g, s))
    # the free run, a move at a time: (result, move, state) and the stream after each move
    free = [[] for _ in range(n)]
    stream_after = [[a.eng.get_rng_state(g)] for g in range(n)]
    for _ in range(total):
        r = a.run(1).clone()
        s, m = a._run_states.clone(), a._run_moves.clone()
        for g in range(n):
            free[g].append((int(r[0, g]), int(m[0, g]), s[0, g].tolist()))
            stream_after[g].append(a.eng.get_rng_state(g))
    seq = [[] for _ in range(n)]
    finished, carried = 0, 0
    for i, bud in enumerate(budgets + [0]):
        rb = (b.run_pooled(bud, cap, carry=True) if i < len(budgets) else b.drain()).clone()
        sb, mb = b._run_states.clone(), b._run_moves.clone()
        m = (rb != 4).sum(0)
        finished += int(m.sum())
        if i < len(budgets):
            carried = max(carried, int(sum(budgets[: i + 1])) - finished)
        for g in range(n):
            for j in range(int(m[g])):
                seq[g].append((int(rb[j, g]), int(mb[j, g]), sb[j, g].tolist()))
    assert carried > 0 and finished == sum(budgets) and not b.carry_pending
    for g in range(n):
        k = len(seq[g])
        assert k <= total and seq[g] == free[g][:k], g
        got, idx = b.eng.get_rng_state(g)
        exp, eidx = stream_after[g][k]
        assert idx == eidx and np.array_equal(got, exp), (g, k)
    a.close()
    b.close()


@pytest.mark.parametrize("bs", [8, 32])
def test_walk_replay_skips_the_recorded_words(eng, bs):
    """zc_debug_c4_walk_async: the search with its rollouts recorded, then replayed from the
    same streams with the rollout words skipped (lrng_skip) — the same move, root visit
    counts, expansions, depth sum and words as the plain search, and the same stream after."""
    from zeroclone_amd import _native
    n, sims = 8, 64
    starts = STARTS[8:16]
    boards = mixed_boards(n, 500 + bs)
    mts = [mt_at(7000 + 13 * g + bs, s) for g, s in enumerate(starts)]
    for g, mt in enumerate(mts):
        put(eng, g, mt)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    nfl = (sims + bs - 1) // bs
    vals = torch.zeros((n, sims), dtype=torch.int8, device=dev)
    words = torch.zeros((n, nfl), dtype=torch.int32, device=dev)
    snap = torch.zeros(n * (4096 * 4 + 16), dtype=torch.uint8, device=dev)
    roots = torch.from_numpy(states(boards).view(np.int64).reshape(n, 3).copy()).to(dev)

    def outs():
        return (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, 7), dtype=torch.int32, device=dev),
                torch.zeros((n, _native.STATS_FIELDS), dtype=torch.int64, device=dev))

    eng.rng_copy(0, n, snap.data_ptr(), False, s)
    runs, streams = [], []
    for mode in (1, 2):
        eng.rng_copy(0, n, snap.data_ptr(), True, s)
        o = outs()
        eng.c4_walk_async(0, n, roots.data_ptr(), sims, 1.4, bs, mode, vals.data_ptr(), words.data_ptr(),
                          o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), s)
        torch.cuda.synchronize(dev)
        runs.append(o)
        streams.append([eng.get_rng_state(g) for g in range(n)])
    ref = oracle_moves(boards, mts, sims, bs)
    for o in runs:
        check_search(o[0].cpu().numpy(), o[1].cpu().numpy(), ref, bs)
    for k in (0, 1, 2, 4, 5):   # expansions, depth sum, leaves, words consumed, status
        assert torch.equal(runs[0][2][:, k], runs[1][2][:, k]), k
    for g, mt in enumerate(mts):
        for got, idx in (streams[0][g], streams[1][g]):
            words_o, index_o = mt.state()
            assert idx == index_o and np.array_equal(got, np.asarray(words_o, np.uint32)), (bs, starts[g])
