"""Tree reuse of the Connect4 PUCT search, without a device: the specification's own rules
(tests/puct_reuse_ref.py), the argument checks of zc_c4_puct_begin_reuse / zc_c4_puct_forget
and of C4SelfPlay(reuse_tree=True)."""
import ctypes

import numpy as np
import pytest

import oracle
from oracle import puct_ref
import puct_reuse_ref as spec
from c4_values import bits_from_rows, hash_value

EMPTY = "." * 42


def _hv(s):
    s0, s1 = bits_from_rows(s[0])
    return hash_value(s0, s1, s[1])


def _uniform(node):
    return [float(np.float32(1.0) / np.float32(len(node.moves)))] * len(node.moves)


def _searched(state, sims=65, bs=8, c=1.5):
    root = puct_ref.Node(state, puct_ref.C4Rules)
    spec.search(root, sims, bs, c, _hv, _uniform)
    return root


def test_fresh_spec_search_is_puct_ref_search():
    s = oracle.play(*oracle.play(EMPTY, 0, 3), 2)
    want = puct_ref.search(s, 65, 8, 1.5, _hv, _uniform, rules=puct_ref.C4Rules)
    root = puct_ref.Node(s, puct_ref.C4Rules)
    assert spec.search(root, 65, 8, 1.5, _hv, _uniform) == want


def test_advance_finds_one_and_two_ply_descendants_only():
    root = _searched((EMPTY, 0))
    j = max(range(len(root.N)), key=lambda k: root.N[k])
    child = root.child[j]
    assert spec.advance(root, child.s) is child
    k = max(range(len(child.N)), key=lambda m: child.N[m])
    gc = child.child[k]
    assert gc.evaluated and spec.advance(root, gc.s) is gc
    assert spec.advance(root, root.s) is None                       # the same position again
    ggc = next(x for x in gc.child if x is not None)
    assert spec.advance(root, ggc.s) is None                        # three plies down
    assert spec.advance(root, oracle.play(*oracle.play(EMPTY, 1, 0), 0)) is None   # not in the tree
    # a child that was created but never evaluated, and a slot without a child
    bare = puct_ref.Node((EMPTY, 0), puct_ref.C4Rules)
    bare.evaluated = True
    s1 = puct_ref.C4Rules.play(bare.s, bare.moves[0])
    bare.child[0] = puct_ref.Node(s1, puct_ref.C4Rules)
    assert spec.advance(bare, s1) is None
    assert spec.advance(bare, puct_ref.C4Rules.play(bare.s, bare.moves[1])) is None


def test_reused_spec_search_adds_sims_minus_one_visits():
    sims = 65
    root = _searched((EMPTY, 0), sims)
    assert sum(root.N) == sims - 1
    j = max(range(len(root.N)), key=lambda k: root.N[k])
    nr, kept = spec.next_root(root, root.child[j].s, sims, 401)
    assert nr is root.child[j] and kept == spec.count_nodes(nr) and kept > 1
    before = sum(nr.N)
    # the edge's first visit was the child's own evaluation (and so is any visit that met it
    # still waiting for that evaluation)
    assert 0 < before <= root.N[j] - 1
    spec.search(nr, sims, 8, 1.5, _hv, _uniform, reused=True)
    assert sum(nr.N) == before + sims - 1
    assert spec.count_nodes(nr) <= kept + sims - 1
    # no room for the kept nodes and a search's own: a fresh root
    fresh, k0 = spec.next_root(root, root.child[j].s, sims, sims + 1)
    assert k0 == 0 and fresh is not root.child[j] and sum(fresh.N) == 0


def test_compact_remaps_a_hand_built_tree():
    from zeroclone_amd._native import C4_PNODE_DTYPE
    #        0
    #      1   2          new root: 2 -> kept 2, 4, 5 (child of 4); 1 and 3 go
    #      3   4
    #          5
    d = np.zeros(6, C4_PNODE_DTYPE)
    d["child"][:] = 0xFFFF
    parent = [0xFFFF, 0, 0, 1, 2, 4]
    pact = [0xFF, 0, 1, 2, 3, 0]
    depth = [0, 1, 1, 2, 2, 3]
    for i in range(6):
        d["parent"][i], d["pact"][i], d["depth"][i] = parent[i], pact[i], depth[i]
        d["s0"][i] = 100 + i
        d["na"][i] = np.arange(8) + 10 * i
        d["w"][i] = -0.5 * i
        d["pr"][i] = 0.125 * i
        if i:
            d["child"][parent[i]][pact[i]] = i
    out = spec.compact(d, 2)
    assert out["s0"].tolist() == [102, 104, 105]
    assert out["parent"].tolist() == [0xFFFF, 0, 1]
    assert out["pact"].tolist() == [0xFF, 3, 0]
    assert out["depth"].tolist() == [0, 1, 2]
    assert out["child"][0].tolist() == [0xFFFF] * 3 + [1] + [0xFFFF] * 4
    assert out["child"][1].tolist() == [2] + [0xFFFF] * 7
    assert (out["child"][2] == 0xFFFF).all()
    for f in ("na", "w", "pr"):
        assert np.array_equal(out[f], d[f][[2, 4, 5]])
    assert d["parent"].tolist() == parent   # a pure function: the input is untouched
    leaf = spec.compact(d, 3)
    assert len(leaf) == 1 and int(leaf["parent"][0]) == 0xFFFF and int(leaf["depth"][0]) == 0


def test_reuse_calls_refuse_a_null_engine_and_one_simulation():
    from zeroclone_amd import _native
    L = _native.lib()
    roots = np.zeros(1, _native.C4_STATE_DTYPE)
    p = ctypes.c_void_p(roots.ctypes.data)
    for sims in (65, 1):   # a null engine, and fewer than two simulations: no device is touched
        rc = L.zc_c4_puct_begin_reuse(None, 0, 1, p, sims, 1.5, 8, 0.3, 0.25, 0, None, None, None)
        assert rc == _native.ZC_EINVAL
    assert L.zc_c4_puct_forget(None, 0, 1, None) == _native.ZC_EINVAL


def test_selfplay_reuse_arguments_are_checked_before_any_engine():
    from zeroclone_amd.selfplay import C4SelfPlay
    with pytest.raises(ValueError, match="puct_net"):
        C4SelfPlay(4, 33, batch_size=8, reuse_tree=True)
    with pytest.raises(ValueError, match="16 bits"):
        C4SelfPlay(4, 1600, batch_size=32, puct_net=object(), reuse_tree=True, record_policy=True)
