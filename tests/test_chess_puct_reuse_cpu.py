"""Tree reuse of the chess PUCT search, without a device: the specification's own rules
(tests/chess_puct_reuse_ref.py), the argument checks of zc_chess_puct_begin_reuse /
zc_chess_puct_forget and of ChessSelfPlay(reuse_tree=True)."""
import ctypes

import numpy as np
import pytest

import oracle
from oracle import puct_ref
import chess_puct_reuse_ref as spec
from test_gpu_puct import FENS, hv

M = 401


def _hv(s):
    return hv(bytes(bytearray(s.board)[:64]), int(s.turn))


def _uniform(node):
    return [float(np.float32(1.0) / np.float32(len(node.moves)))] * len(node.moves)


@pytest.mark.parametrize("fen", FENS[:4])
def test_spec_sequence_reuses_and_adds_sims_minus_one_visits(fen):
    """Five searches at sims 65, bs 8, c 1.5 along the most-visited line: the first is fresh,
    the other four keep a subtree of 5 to 33 nodes, and every search adds sims - 1 visits."""
    sims, bs, c = 65, 8, 1.5
    state, root, kepts = oracle.chess_from_fen(fen), None, []
    for t in range(5):
        root, kept = spec.next_root(root, state, sims, M)
        before = sum(root.N)
        assert (kept == 0) == (before == 0 and not root.evaluated)
        moves, N, best = spec.search(root, sims, bs, c, _hv, _uniform, rules=puct_ref.ChessRules, reused=kept > 0)
        assert sum(N) == before + sims - 1
        assert spec.count_nodes(root) <= (kept or 1) + sims - 1
        kepts.append(kept)
        state = oracle.chess_play(state, moves[best])
    assert kepts[0] == 0 and all(5 <= k <= 33 for k in kepts[1:]), kepts


def test_fresh_spec_search_is_puct_ref_search():
    s = oracle.chess_from_fen(FENS[3])
    want = puct_ref.search(s, 40, 8, 1.5, _hv, _uniform)
    root = puct_ref.Node(s, puct_ref.ChessRules)
    assert spec.search(root, 40, 8, 1.5, _hv, _uniform, rules=puct_ref.ChessRules) == want


def test_advance_and_both_halves_of_the_room_rule():
    sims = 65
    s = oracle.chess_from_fen(FENS[0])
    root = puct_ref.Node(s, puct_ref.ChessRules)
    spec.search(root, sims, 8, 1.5, _hv, _uniform, rules=puct_ref.ChessRules)
    j = max(range(len(root.N)), key=lambda k: (root.N[k], -k))
    child = root.child[j]
    assert spec.advance(root, spec.key(child.s)) is child
    assert spec.advance(root, spec.key(root.s)) is None            # the same position again
    gc = next(x for x in child.child if x is not None and x.evaluated and x.moves)
    assert spec.advance(root, spec.key(gc.s)) is gc
    ggc = next((x for x in gc.child if x is not None), None)
    if ggc is not None:
        assert spec.advance(root, spec.key(ggc.s)) is None         # three plies down
    assert spec.advance(root, spec.key(oracle.chess_from_fen(FENS[2]))) is None   # not in the tree
    bare = puct_ref.Node(s, puct_ref.ChessRules)   # a child created but never evaluated, a slot without a child
    bare.evaluated = True
    s1 = oracle.chess_play(s, bare.moves[0])
    bare.child[0] = puct_ref.Node(s1, puct_ref.ChessRules)
    assert spec.advance(bare, spec.key(s1)) is None
    assert spec.advance(bare, spec.key(oracle.chess_play(s, bare.moves[1]))) is None
    # fifty and castle are part of the key, the reserved bytes are not
    k = spec.key(child.s)
    assert spec.advance(root, (k[0], k[1], k[2] + 1, k[3])) is None
    assert spec.advance(root, (k[0], k[1], k[2], k[3] ^ 1)) is None
    kept, slots = spec.count_nodes(child), spec.count_slots(child)
    assert kept > 1 and slots >= len(child.moves)
    # kept + sims - 1 <= M and kept_slots + 64 * (sims - 1) <= 64 * M: the smallest M with both
    assert spec.next_root(root, child.s, sims, kept + sims - 2)[1] == 0
    m_min = max(-(-(slots + 64 * (sims - 1)) // 64), kept + sims - 1)
    assert spec.next_root(root, child.s, sims, m_min)[1] == kept
    assert spec.next_root(root, child.s, sims, m_min - 1)[1] == 0


def test_compact_remaps_a_hand_built_dump():
    from zeroclone_amd._native import CHESS_NODE_DTYPE
    #        0
    #      1   2          new root: 2 -> kept 2, 4, 5 (child of 4); 1 and 3 go
    #      3   4
    #          5
    parent = [0xFFFF, 0, 0, 1, 2, 4]
    pact = [0xFFFF, 0, 1, 2, 1, 0]
    depth = [0, 1, 1, 2, 2, 3]
    nmoves = [3, 4, 2, 0, 70, 1]
    base = [0, 3, 7, 9, 9, 79]
    nodes = np.zeros(6, CHESS_NODE_DTYPE)
    S = 80
    d = {"nodes": nodes, "mv": np.arange(S, dtype=np.uint16) + 1000, "prior": np.arange(S, dtype=np.float32) / 128,
         "na": np.arange(S, dtype=np.int32) * 3, "w": -0.5 * np.arange(S, dtype=np.float64),
         "child": np.full(S, 0xFFFF, np.uint16)}
    for i in range(6):
        nodes["parent"][i], nodes["pact"][i], nodes["depth"][i] = parent[i], pact[i], depth[i]
        nodes["nmoves"][i], nodes["base"][i], nodes["st"][i][0] = nmoves[i], base[i], 100 + i
        nodes["evaluated"][i] = 1
        if i:
            d["child"][base[parent[i]] + pact[i]] = i
    keep = {f: d[f].copy() for f in d if f != "nodes"}
    out = spec.compact(d, 2)
    on = out["nodes"]
    assert on["st"][:, 0].tolist() == [102, 104, 105]
    assert on["parent"].tolist() == [0xFFFF, 0, 1]
    assert on["pact"].tolist() == [0xFFFF, 1, 0]
    assert on["depth"].tolist() == [0, 1, 2]
    assert on["nmoves"].tolist() == [2, 70, 1] and on["base"].tolist() == [0, 2, 72]
    old_slots = list(range(7, 9)) + list(range(9, 79)) + [79]
    for f in ("mv", "prior", "na", "w"):
        assert out[f].tobytes() == d[f][old_slots].tobytes(), f
    want_child = [0xFFFF] * 73
    want_child[1] = 1        # node 2's slot 1 -> old 4 -> new 1
    want_child[2 + 0] = 2    # old 4's slot 0 -> old 5 -> new 2
    assert out["child"].tolist() == want_child
    assert nodes["parent"].tolist() == parent and all((d[f] == keep[f]).all() for f in keep)   # a pure function
    leaf = spec.compact(d, 3)
    assert len(leaf["nodes"]) == 1 and int(leaf["nodes"]["parent"][0]) == 0xFFFF and len(leaf["mv"]) == 0
    assert spec.find(d, spec.dump_key(d, 2)) == 2 and spec.find(d, spec.dump_key(d, 4)) == 4
    assert spec.find(d, spec.dump_key(d, 5)) is None      # three plies down
    assert spec.find(d, spec.dump_key(d, 3)) is None      # no moves
    assert spec.find(d, spec.dump_key(d, 0)) is None      # the root itself


def test_reuse_calls_refuse_a_null_engine_and_one_simulation():
    from zeroclone_amd import _native
    L = _native.lib()
    roots = np.zeros(1, _native.CHESS_STATE_DTYPE)
    p = ctypes.c_void_p(roots.ctypes.data)
    for sims in (65, 1):   # a null engine, and fewer than two simulations: no device is touched
        rc = L.zc_chess_puct_begin_reuse(None, 0, 1, p, sims, 1.5, 8, 0.3, 0.25, 0, None, None, None)
        assert rc == _native.ZC_EINVAL
    assert L.zc_chess_puct_forget(None, 0, 1, None) == _native.ZC_EINVAL


def test_selfplay_reuse_needs_the_puct_network_before_any_engine():
    from zeroclone_amd.selfplay import ChessSelfPlay
    with pytest.raises(ValueError, match="puct_net"):
        ChessSelfPlay(4, 33, batch_size=8, reuse_tree=True)
