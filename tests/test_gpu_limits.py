"""The searches at the limits the C-ABI declares (zc_engine_create: max_sims <= 65533, max_batch
<= 512, 256 for the fused crude chess search), against the oracle, the reference's limit goldens
(tests/golden/gen_golden_limits.py) and the PUCT specification.  What these shapes reach and the
workload shapes do not:

* the Connect4 rollout kernels with two waves per workgroup (batch 315..512; four up to 314,
  where the workgroup takes 163,584 of the CU's 163,840 bytes of LDS), ragged last workgroups;
* flushes of more than 100 leaves in select_flush, of 129..256 leaves in the crude chess backup;
* node ids from 32768 up in every tree, chess child slots from 65536 up.

Each test states how it knows that it reached its regime."""
import random
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import oracle
from c4_philox_ref import value_batch as philox_value_batch
from c4_positions import EMPTY, deep_leaning_roots, opening, states
from c4_values import bits_from_rows, hash_value

pytestmark = pytest.mark.gpu

TOP = 65533   # the largest max_sims: node ids are uint16, 0xFFFF is "none"
SKIP, ONGOING = 4, 2


def _engine(**kw):
    from zeroclone_amd._native import NativeEngine
    return NativeEngine(**kw)


@pytest.fixture(scope="module")
def wide():
    """1100 simulations at any batch size."""
    e = _engine(max_games=67, max_sims=1100, max_batch=512)
    yield e
    e.close()


@pytest.fixture(scope="module")
def top():
    """The top of the simulation range at the largest batch."""
    e = _engine(max_games=5, max_sims=TOP, max_batch=512)
    yield e
    e.close()


@pytest.fixture(scope="module")
def chess_top():
    e = _engine(max_games=3, max_sims=TOP, max_batch=256)
    yield e
    e.close()


def _mixed_roots(n, seed):
    """The empty board, openings of up to 14 plies and the deep, leaning roots of
    test_gpu_c4.test_planned_flush_deep_roots_match_oracle, about a third each."""
    rng = random.Random(seed)
    k = n // 3
    return ([(EMPTY, 0)] * (n - 2 * k) + [opening(rng, 14) for _ in range(k)] + deep_leaning_roots(rng, k))[:n]


def _python_next_word(eng, game):
    mt, idx = eng.get_rng_state(game)
    r = random.Random()
    r.setstate((3, tuple(int(x) for x in mt) + (idx,), None))
    return r.getrandbits(32)


def _c4_against_oracle(eng, boards, seeds, sims, bs):
    """The suite's comparison: move, root visits, words drawn, leaves, status.  Returns the stats."""
    eng.seed(0, seeds)
    mv, na, st = eng.c4_search(states(boards), sims, 1.4, bs)
    omv, ona, ocons = oracle.get_move_batch([b for b, _ in boards], [t for _, t in boards], seeds, sims, 1.4, bs,
                                            threads=16)
    assert np.array_equal(mv, omv)
    assert np.array_equal(na, ona)
    assert np.array_equal(st["rng_words"], ocons.astype(np.int64))
    assert (st["leaves"] == sims).all() and (st["status"] == 0).all()
    return st


# ------------------------------------------------------------------ a. workgroup regimes
@pytest.mark.parametrize("bs", [128, 200, 314, 315, 512])
def test_c4_search_across_workgroup_regimes(wide, bs):
    """67 games (1 mod 2 and 3 mod 4: the last workgroup is ragged with four waves and with two)
    of 1100 simulations: several whole flushes of more than 100 leaves and a partial last one at
    every batch size."""
    n, sims = 67, 1100
    assert n % 4 and n % 2 and sims % bs and sims // bs >= 2
    _c4_against_oracle(wide, _mixed_roots(n, 67), [1_000_003 * g + bs for g in range(n)], sims, bs)


@pytest.mark.parametrize("bs", [315, 512])
def test_c4_philox_search_with_two_waves_per_workgroup(wide, bs):
    """The same games in the Philox rollout mode against its specification (c4_philox_ref), as
    test_gpu_philox does at batch 8..64."""
    n, sims, seed = 67, 1100, 0x5EED_0C4F_2024
    boards = _mixed_roots(n, 67)
    seeds = [31 + 7 * i for i in range(n)]
    wide.c4_rollout_mode("philox", seed)
    try:
        wide.seed(0, seeds)
        mv, na, st = wide.c4_search(states(boards), sims, 1.4, bs)
    finally:
        wide.c4_rollout_mode("exact")
    assert (st["leaves"] == sims).all() and (st["status"] == 0).all()
    for i, (board, turn) in enumerate(boards):
        mt = oracle.MT(seeds[i])
        col, rna, order = oracle.get_move_valued(board, turn, mt, sims, 1.4, bs, philox_value_batch(624, i, seed))
        assert [int(na[i, c]) for c in order] == rna, i
        assert int(mv[i]) == col
        assert int(st["rng_words"][i]) == mt.drawn   # expansion draws only


@pytest.mark.parametrize("bs", [315, 512])
def test_c4_walk_diagnostic_with_two_waves_per_workgroup(wide, bs):
    """c4_walk_kernel (zc_debug_c4_walk_async) shares the search's workgroup shape: the run that
    records the rollouts and the one that replays them from the same seeds both equal the oracle."""
    from zeroclone_amd import _native
    n, sims = 67, 1100
    boards = _mixed_roots(n, 67)
    seeds = [424_243 * g + bs for g in range(n)]
    omv, ona, ocons = oracle.get_move_batch([b for b, _ in boards], [t for _, t in boards], seeds, sims, 1.4, bs,
                                            threads=16)
    roots = torch.from_numpy(states(boards).view(np.int64).reshape(n, 3).copy()).cuda()
    vals = torch.zeros((n, sims), dtype=torch.int8, device="cuda")
    words = torch.zeros((n, (sims + bs - 1) // bs), dtype=torch.int32, device="cuda")
    for mode in (1, 2):
        wide.seed(0, seeds)
        mv = torch.zeros(n, dtype=torch.int32, device="cuda")
        na = torch.zeros((n, 7), dtype=torch.int32, device="cuda")
        st = torch.zeros((n, _native.STATS_FIELDS), dtype=torch.int64, device="cuda")
        wide.c4_walk_async(0, n, roots.data_ptr(), sims, 1.4, bs, mode, vals.data_ptr(), words.data_ptr(),
                           mv.data_ptr(), na.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        st = st.cpu().numpy()
        assert np.array_equal(mv.cpu().numpy(), omv), mode
        assert np.array_equal(na.cpu().numpy(), ona), mode
        assert np.array_equal(st[:, 4], ocons.astype(np.int64)), mode
        assert (st[:, 2] == sims).all() and (st[:, 5] == 0).all(), mode


# ------------------------------------------------------------------ b. the reference's limit goldens
def test_c4_limit_goldens_on_the_device(wide, top, golden):
    cases = golden("c4_get_move_limits.json")["cases"]
    groups = defaultdict(list)
    for c in cases:
        groups[(c["sims"], c["bs"], c["c"])].append(c)
    assert {(TOP, 32), (TOP, 512), (1100, 314), (1100, 315), (1100, 512)} <= {k[:2] for k in groups}
    for (sims, bs, cc), cs in groups.items():
        eng = top if sims > wide.max_sims else wide
        eng.seed(0, [c["seed"] for c in cs])
        mv, na, st = eng.c4_search(states([(c["board"], c["turn"]) for c in cs]), sims, cc, bs)
        for i, c in enumerate(cs):
            assert [int(na[i][col]) for col in c["order"]] == c["root_na"], (c["seed"], sims, bs)
            assert int(mv[i]) == c["move"]
            assert int(st[i]["rng_words"]) == c["consumed"]
            assert int(st[i]["leaves"]) == sims == c["leaves"] and int(st[i]["status"]) == 0
            assert _python_next_word(eng, i) == c["next_word"]


def _crude(eng, fens, seeds, sims, bs):
    from test_gpu_chess_search import MAXM, roots_of
    from zeroclone_amd._native import ZC_POLICY_IMMEDIATE_VALUE
    n = len(fens)
    eng.seed(0, seeds)
    roots = roots_of(fens)
    mv = torch.zeros(n, dtype=torch.int16, device="cuda")
    na = torch.zeros((n, MAXM), dtype=torch.int32, device="cuda")
    st = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    eng.chess_search_async(0, n, roots.data_ptr(), sims, 1.4, bs, ZC_POLICY_IMMEDIATE_VALUE, 3.0, mv.data_ptr(),
                           na.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    return mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy()


def test_chess_limit_goldens_on_the_device(chess_top, golden):
    from test_gpu_chess_search import decode
    groups = defaultdict(list)
    for c in golden("chess_get_move_limits.json")["cases"]:
        assert (c["c"], c["policy"], c["freedom"]) == (1.4, "immediate_value", 3)
        groups[(c["sims"], c["bs"])].append(c)
    assert {(400, 129), (400, 256), (TOP, 64), (TOP, 256)} <= set(groups)
    for (sims, bs), grp in groups.items():
        mv, na, st = _crude(chess_top, [c["fen"] for c in grp], [c["seed"] for c in grp], sims, bs)
        for i, c in enumerate(grp):
            k = len(c["root_moves"])
            assert st[i, 5] == 0, (c["fen"], st[i])
            assert list(na[i, :k]) == c["root_na"], (c["fen"], sims, bs)
            assert decode(mv[i]) == c["move"]
            assert st[i, 4] == c["consumed"] and st[i, 2] == sims == c["leaves"]
            assert _python_next_word(chess_top, i) == c["next_word"]


# ------------------------------------------------------------------ c. top of the simulation range
def test_c4_top_of_the_simulation_range(top):
    """65533 simulations from the empty board and from openings of at most 8 plies, at batch 32
    and 512.  At batch 32 every simulation makes a node (by the oracle on the CPU: 65,534 nodes a
    game), so the ids cross 15 bits and end at 0xFFFD; at batch 512 a flush piles onto one chain
    whose terminal leaves make no nodes, and the same roots give trees of about 20,000 nodes."""
    rng = random.Random(TOP)
    boards = [(EMPTY, 0)] + [opening(rng, 8) for _ in range(4)]
    nodes = []
    for bs in (32, 512):
        st = _c4_against_oracle(top, boards, [9000 + 11 * g + bs for g in range(5)], TOP, bs)
        nodes += [int(x) + 1 for x in st["expansions"]]
    print("nodes per tree:", nodes)
    assert max(nodes) > 60_000   # else the test never left 15-bit node ids


def test_max_sims_past_the_node_id_range_is_refused():
    with pytest.raises(ValueError):
        _engine(max_games=1, max_sims=TOP + 1, max_batch=32)


# ------------------------------------------------------------------ d. self-play, two waves per workgroup
def _board_of(row):
    s0, s1, t = (int(x) for x in row)
    cells = []
    for r in range(6):
        for c in range(7):
            bit = 1 << (7 * c + (5 - r))
            cells.append("X" if s0 & bit else ("O" if s1 & bit else "."))
    return "".join(cells), t & 1


def _oracle_mt(eng, g):
    mt, idx = eng.get_rng_state(g)
    o = oracle.MT(0)
    o.s.mt[:] = [int(x) for x in mt]
    o.s.index = idx
    return o


def _replay(eng, snap_roots, mts, sims, bs, states_, moves, results):
    """test_gpu_headline.replay at this file's shapes: every game's moves through the oracle from
    the snapshotted roots and MT states; the device streams must end where the oracle's do."""
    checked = 0
    K, G = results.shape
    for g in range(G):
        b, t = _board_of(snap_roots[g])
        mt = mts[g]
        for k in range(K):
            r = int(results[k, g])
            if r == SKIP:
                assert (results[k:, g] == SKIP).all(), g   # a game's moves are a prefix of the steps
                break
            col, _, _ = oracle.get_move_mt(b, t, mt, sims, 1.4, bs)
            assert int(moves[k, g]) == col, (g, k)
            b, t = oracle.play(b, t, col)
            assert _board_of(states_[k, g]) == (b, t), (g, k)
            exp = t * 2 - 1 if oracle.check_win(b, t) else (0 if oracle.check_draw(b) else ONGOING)
            assert r == exp, (g, k, r, exp)
            if exp != ONGOING:
                b, t = EMPTY, 0
            checked += 1
        mt_dev, idx_dev = eng.get_rng_state(g)
        assert [int(x) for x in mt_dev] == list(mt.s.mt) and idx_dev == mt.s.index, g
    return checked


@pytest.mark.parametrize("bs", [315, 512])
def test_c4_selfplay_kernels_with_two_waves_per_workgroup(bs):
    """C4SelfPlay(37 games: a ragged last workgroup, 600 simulations): three lockstep steps, a
    pooled launch, then carry launches and their drain, every move replayed through the oracle
    as test_gpu_headline does at the headline shape, the MT states included."""
    from zeroclone_amd.selfplay import C4SelfPlay
    G, S = 37, 600
    assert G % 2
    sp = C4SelfPlay(G, S, batch_size=bs, seed=315, record=True)
    try:
        snap = sp.roots.cpu().numpy().copy()
        mts = [_oracle_mt(sp.eng, g) for g in range(G)]
        res, sts, mvs = [], [], []
        for _ in range(3):   # lockstep; no game ends within three moves
            res.append(sp.step().cpu().numpy().copy())
            sts.append(sp.roots.cpu().numpy().copy())
            mvs.append(sp.moves.cpu().numpy().copy())
        assert (np.array(res) == ONGOING).all() and int(sp.stats[:, 5].abs().sum()) == 0
        assert _replay(sp.eng, snap, mts, S, bs, np.array(sts), np.array(mvs), np.array(res)) == 3 * G

        snap = sp.roots.cpu().numpy().copy()
        mts = [_oracle_mt(sp.eng, g) for g in range(G)]
        res = sp.run_pooled(3 * G, 6).cpu().numpy()
        assert int((res != SKIP).sum()) == 3 * G and int(sp.stats[:, 5].abs().sum()) == 0
        assert _replay(sp.eng, snap, mts, S, bs, sp._run_states.cpu().numpy(), sp._run_moves.cpu().numpy(),
                       res) == 3 * G

        snap = sp.roots.cpu().numpy().copy()
        mts = [_oracle_mt(sp.eng, g) for g in range(G)]
        parts = []
        for k in (3, 2, None):
            r = (sp.run_pooled(k * G, 2 * k, carry=True) if k else sp.drain()).cpu().numpy()
            parts.append((r, sp._run_states.cpu().numpy(), sp._run_moves.cpu().numpy()))
            assert int(sp.stats[:, 5].abs().sum()) == 0
        played = [(r != SKIP).sum(0) for r, _, _ in parts]
        assert int(sum(p.sum() for p in played)) == 5 * G   # every ticketed move finished once
        K = sum(r.shape[0] for r, _, _ in parts)
        res_all = np.full((K, G), SKIP, np.int32)
        st_all = np.zeros((K, G, 3), np.int64)
        mv_all = np.zeros((K, G), np.int16)
        for g in range(G):   # a game's finished moves in order: launch 1's prefix, launch 2's, the drain's
            row = 0
            for (r, st, mv), cnt in zip(parts, played):
                c = int(cnt[g])
                res_all[row:row + c, g], st_all[row:row + c, g], mv_all[row:row + c, g] = r[:c, g], st[:c, g], mv[:c, g]
                row += c
        assert _replay(sp.eng, snap, mts, S, bs, st_all, mv_all, res_all) == 5 * G
        assert not sp.carry_pending
    finally:
        sp.close()


@pytest.mark.parametrize("bs,waves", [(314, 4), (315, 2), (512, 2)])
def test_pooled_capacity_counts_whole_workgroups(wide, bs, waves):
    """zc_c4_pooled_max_games = resident workgroups x the waves per workgroup of the launch (four
    up to batch 314, two from 315: c4_search.hip's c4_search_wpg)."""
    cap = wide.c4_pooled_max_games(bs)
    assert cap > 0 and cap % waves == 0, cap


# ------------------------------------------------------------------ e. the stepwise (valued) search
def _hash_rows(leaves, planes, counts):
    """c4_values.hash_value of every leaf row, in uint64 arithmetic (which wraps as the & M64)."""
    r = leaves.cpu().numpy().view(np.uint64)
    with np.errstate(over="ignore"):
        h = (r[:, 0] * np.uint64(0x9E3779B97F4A7C15) + r[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F)
             + (r[:, 2] & np.uint64(1)) * np.uint64(0x165667B19E3779F9))
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    out = ((h % np.uint64(200001)).astype(np.int64) - 100000) / 100003.0
    k = min(8, len(r))
    assert [float(x) for x in out[:k]] == [hash_value(int(x[0]), int(x[1]), int(x[2]) & 1) for x in r[:k]]
    return torch.from_numpy(out).cuda()


def _hash_batch(boards, turns):
    return [hash_value(*bits_from_rows(b), t) for b, t in zip(boards, turns)]


def _valued_against_oracle(eng, boards, seeds, sims, bs):
    from zeroclone_amd.valued import C4ValuedSearch
    n = len(boards)
    eng.seed(0, seeds)
    roots = torch.from_numpy(states(boards).view(np.int64).reshape(n, 3).copy()).cuda()
    mv, na, st = C4ValuedSearch(eng, n, bs, planes=False).run(roots, sims, 1.4, _hash_rows)
    mv, na, st = mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy()
    for i, (b, t) in enumerate(boards):
        mt = oracle.MT(seeds[i])
        col, rna, order = oracle.get_move_valued(b, t, mt, sims, 1.4, bs, _hash_batch)
        assert [int(na[i, c]) for c in order] == rna, i
        assert int(mv[i]) == col
        assert st[i, 4] == mt.drawn and st[i, 2] == sims and st[i, 5] == 0
    return st


@pytest.mark.parametrize("bs", [129, 256, 512])
def test_stepwise_search_with_large_flushes(wide, bs):
    """c4_ext.hip (2048 + 168 * bs + 64 bytes of LDS: 88 KB at batch 512) with the hash value of
    c4_values, against the oracle's valued get_move."""
    n = 9
    _valued_against_oracle(wide, _mixed_roots(n, 129), [77 * g + bs for g in range(n)], 1100, bs)


def test_stepwise_search_at_the_top_of_the_simulation_range(top):
    """65533 simulations in 128 flushes of 512, whose chains end in terminal leaves after about
    20,000 nodes, and in 2048 flushes of 32, where nearly every simulation makes a node (by the
    oracle on the CPU some 500 to 2,600 leaves of such a game are terminal), so the uint16 path entries and
    links of this search cross 15 bits too."""
    boards = [(EMPTY, 0), opening(random.Random(4), 8)]
    nodes = []
    for bs in (512, 32):
        st = _valued_against_oracle(top, boards, [51 + bs, 52 + bs], TOP, bs)
        nodes += [int(x) + 1 for x in st[:, 0]]
    print("nodes per tree:", nodes)
    assert max(nodes) > 60_000


# ------------------------------------------------------------------ f. the crude chess search
KIWIPETE = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
MIDDLEGAMES = [KIWIPETE, "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8",
               "r1bq1rk1/2p1bppp/p1np1n2/1p2p3/4P3/1BP2N1P/PP1P1PP1/RNBQR1K1 b - - 0 9"]
ENDGAMES = ["8/8/3k4/8/8/3K4/3Q4/8 w - - 0 1", "6k1/5ppp/8/8/8/8/5PPP/3R2K1 w - - 0 1",
            "8/8/8/4k3/8/8/8/R3K3 w - - 0 1", "7k/8/8/8/8/8/8/K6Q w - - 0 1"]


def _oracle_crude(fen, seed, sims, bs):
    mt = oracle.MT(seed)
    best, moves, rna = oracle.chess_get_move(oracle.chess_from_fen(fen), mt, sims, 1.4, bs, "immediate_value", 3.0)
    return list(moves[best]), len(moves), rna, mt.drawn, oracle.chess_last_tree()


@pytest.fixture(scope="module")
def chess_wide():
    e = _engine(max_games=12, max_sims=400, max_batch=512)
    yield e
    e.close()


@pytest.mark.parametrize("bs", [129, 200, 256])
def test_crude_search_flushes_past_128_leaves(chess_wide, bs):
    """The leaf-by-leaf backup of chess_search.hip at 129 to 256 leaves a flush, on the positions
    of test_gpu_chess_search.test_crude_search_large_flushes_match_oracle."""
    from test_gpu_chess_search import FENS, decode
    fens = FENS * 2 + ENDGAMES
    n, sims = len(fens), 400
    seeds = [90 + i + bs for i in range(n)]
    mv, na, st = _crude(chess_wide, fens, seeds, sims, bs)
    for i, fen in enumerate(fens):
        move, k, rna, drawn, _ = _oracle_crude(fen, seeds[i], sims, bs)
        assert st[i, 5] == 0, (fen, st[i])
        assert list(na[i, :k]) == rna, fen
        assert decode(mv[i]) == move, fen
        assert st[i, 4] == drawn and st[i, 2] == sims, fen


def test_crude_search_refuses_257_leaves_a_flush(chess_wide):
    with pytest.raises(ValueError):
        _crude(chess_wide, [KIWIPETE], [1], 400, 257)


@pytest.mark.parametrize("bs", [64, 256])
def test_crude_search_at_the_top_of_the_simulation_range(chess_top, bs):
    """65533 simulations on three middlegames chosen on the CPU: by the oracle their trees stay
    at 19 levels or fewer (the device walks to level 62) and give slots to the 69,000 to 86,000
    legal moves of the nodes they expand, so the slot numbers pass 16 bits."""
    from test_gpu_chess_search import decode
    n = len(MIDDLEGAMES)
    seeds = [5004 + i + bs for i in range(n)]
    with ThreadPoolExecutor(n) as ex:
        want = list(ex.map(lambda i: _oracle_crude(MIDDLEGAMES[i], seeds[i], TOP, bs), range(n)))
    mv, na, st = _crude(chess_top, MIDDLEGAMES, seeds, TOP, bs)
    for i, fen in enumerate(MIDDLEGAMES):
        move, k, rna, drawn, (onodes, oslots, odepth) = want[i]
        assert odepth <= 62 and oslots > 65_536 and onodes > 60_000, (fen, onodes, oslots, odepth)
        assert st[i, 5] == 0, (fen, st[i])
        assert list(na[i, :k]) == rna, fen
        assert decode(mv[i]) == move, fen
        assert st[i, 4] == drawn and st[i, 2] == TOP, fen
        tree = chess_top.debug_chess_tree(i, max_nodes=1 << 16, max_slots=1 << 20)
        print(fen, "nodes", len(tree["nodes"]), "slots", len(tree["mv"]), "oracle", onodes, oslots, odepth)
        assert len(tree["nodes"]) == onodes
        assert len(tree["mv"]) > 65_536   # else no slot number left 16 bits


# ------------------------------------------------------------------ g. PUCT tree reuse across 15 bits
def test_c4_puct_reuse_across_the_15_bit_boundary():
    """32,000 simulations from the empty board, the most visited move, then a reused search of
    33,000 more at batch 512 with the deterministic values and uniform priors of
    test_gpu_c4_puct: by the spec (tests/puct_reuse_ref.py; 6 s on the CPU) the re-root keeps
    11,615 nodes and the second tree ends with 44,069, so the kept records are renumbered and
    the new ids pass 32768."""
    import puct_reuse_ref as spec
    from oracle import puct_ref
    from test_gpu_c4_puct import _hash_net, _hv, _roots
    from zeroclone_amd.valued import C4PuctSearch

    def uniform(node):
        return [float(np.float32(1.0) / np.float32(len(node.moves)))] * len(node.moves)

    bs, c, M = 512, 1.5, TOP + 1
    e = _engine(max_games=1, max_sims=TOP, max_batch=bs)
    try:
        ps = C4PuctSearch(e, 1, bs, c_puct=c, dirichlet_eps=0.0, reuse=True)
        state, root = (EMPTY, 0), None
        for sims in (32_000, 33_000):
            assert puct_ref.C4Rules.moves(state)
            root, kept = spec.next_root(root, state, sims, M)
            kept_visits = sum(root.N)
            moves, N, best = spec.search(root, sims, bs, c, _hv, uniform, reused=kept > 0)
            mv, na, st = ps.run(_roots([state]), sims, _hash_net)
            na, st = na.cpu().numpy(), st.cpu().numpy()
            assert st[0, 5] == 0
            assert int(ps.kept[0]) == kept
            assert [int(na[0, col]) for col in moves] == N
            assert int(mv[0]) == moves[best]
            assert int(na[0].sum()) == kept_visits + sims - 1 == sum(N)
            assert len(e.debug_c4_puct_tree(0)) == spec.count_nodes(root) == (kept or 1) + st[0, 0]
            state = oracle.play(state[0], state[1], moves[best])
        assert kept > 1000 and spec.count_nodes(root) > 40_000
    finally:
        e.close()
