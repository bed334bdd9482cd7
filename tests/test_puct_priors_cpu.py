"""CPU checks of the non-uniform-prior cases of test_gpu_puct_priors.py (tests/puct_prior_cases.py):
(a) each case reaches the edge it is there for, asserted on the specification's own trees — the
two limits of the chess kernel (oracle/puct_ref.py's max_level and slot_cap) included; (b) the
two comparisons the GPU test makes (check_priors, compare_trees) reject six deliberately wrong
searches on the same cases.  The "device" here is the specification itself with the float32
restatement of the softmax (Logits.prior32), so the comparisons also pass on what they should."""
import pytest

import oracle
from oracle import puct_ref
import puct_prior_cases as pc
import puct_reuse_ref

SLOT_SIMS, SLOT_BS, SLOT_CAP = 128, 8, 64 * 129   # a fresh search with sims = max_sims = 128


@pytest.fixture(scope="module")
def runs():
    """case name -> the specification's searches of the case's roots."""
    return {case.name: case.spec() for case in pc.CASES}


def _case(kind, game=pc.Chess, **kw):
    out = [c for c in pc.CASES if c.game is game and c.kind == kind and all(getattr(c, k) == v for k, v in kw.items())]
    assert out
    return out[0]


def test_the_comparisons_accept_the_specification(runs):
    for case in pc.CASES:
        lg = case.logits()
        for r in runs[case.name]:
            assert r.capacity is None and sum(r.N) == case.sims - 1
            pc.check_priors(r.tree, lg, case.name, case.masked_unvisited)
            pc.compare_trees(r.tree, r.tree)
    assert {c.bs for c in pc.CHESS_CASES} == {c.bs for c in pc.C4_CASES} == {1, 8, 32}
    assert {c.c for c in pc.CASES} == {0.7, 1.5, 2.5}
    assert all(c.sims % c.bs or c.bs == 1 for c in pc.CASES) and all(c.sims <= 260 for c in pc.CASES)
    for cases in (pc.CHESS_CASES, pc.C4_CASES):   # both logit types, both rows paths, every kind
        assert {c.half for c in cases} == {c.roots_only for c in cases} == {False, True}
        assert {c.kind for c in cases} == {"hash", "line", "tie", "mask"}
    assert {c.scale for c in pc.CASES if c.kind == "hash"} == {0.05, 3, 12}


def test_peaked_priors_repeat_pending_leaves(runs):
    """A flush of 8 under the line logits walks into its own pending leaf again and again."""
    for game in (pc.Chess, pc.C4):
        case = _case("line", game, bs=8)
        rep = [r.repeats for r in runs[case.name][:3]]   # the start position, kiwipete, pos3 / three open boards
        assert min(rep) >= 15, rep
    flat = _case("hash", scale=0.05)
    assert max(r.repeats for r in runs[flat.name]) <= 3


@pytest.mark.parametrize("bs,last_ok", [(1, 63), (4, 249)])
def test_the_depth_limit_is_reached_exactly(bs, last_ok):
    """The line logits grow the tree one level a flush: the deepest node a search can evaluate is
    at level 62, and the first walk to stand on it ends the search."""
    lg = pc.Logits(pc.Chess, "line", 40)
    for fen in pc.LINE_FENS:
        s = oracle.chess_from_fen(fen)
        ok = pc.SpecRun(lg, s, last_ok, bs, 1.5, max_level=pc.MAX_LEVEL)
        assert ok.capacity is None and max(pc.levels(ok.tree)) == pc.MAX_LEVEL == 62
        over = pc.SpecRun(lg, s, last_ok + 1, bs, 1.5, max_level=pc.MAX_LEVEL)
        assert over.capacity is not None and (over.capacity.kind, over.capacity.flush) == ("depth", 63)
        assert over.flush_counts(last_ok + 1, bs)[62:] == [bs, 0] and len(over.flush_counts(last_ok + 1, bs)) == 64
        free = pc.SpecRun(lg, s, 80, bs, 1.5)   # the specification itself has no such rule
        assert free.capacity is None and max(pc.levels(free.tree)) == (79 if bs == 1 else 20)


def test_wide_and_terminal_nodes_below_the_root(runs):
    wide, one, mates, stale = [], 0, 0, 0
    for case in pc.CHESS_CASES:
        for r in runs[case.name]:
            wide += [len(x["moves"]) for x in r.tree[1:] if x["evaluated"]]
            one += sum(1 for x in r.tree[1:] if x["evaluated"] and len(x["moves"]) == 1)
            for x in r.tree:
                if not x["moves"]:
                    won = oracle.chess_win(pc.Chess.state(x["key"]))
                    mates, stale = mates + won, stale + (not won)
    for lo, hi in ((65, 128), (129, 192), (193, 256)):   # the softmax's chunks 2, 3 and 4 below the root
        assert any(lo <= w <= hi for w in wide), (lo, hi)
    assert one >= 5 and mates >= 1 and stale >= 10, (one, mates, stale)


def test_the_slot_pool_overruns_at_a_known_flush():
    lg = pc.Logits(pc.Chess, "hash", 3)
    s = oracle.chess_from_fen(pc.SLOT_FEN)
    r = pc.SpecRun(lg, s, SLOT_SIMS, SLOT_BS, 1.5, slot_cap=SLOT_CAP)
    assert r.capacity is not None and (r.capacity.kind, r.capacity.flush) == ("slots", 14)
    assert sum(len(x["moves"]) for x in r.tree) > SLOT_CAP and len(r.tree) <= SLOT_SIMS + 1
    counts = r.flush_counts(SLOT_SIMS, SLOT_BS)
    assert counts[:16] == [1] + [8] * 14 + [0] and not any(counts[15:])   # flush 14 selects, nothing after
    free = pc.SpecRun(lg, s, SLOT_SIMS, SLOT_BS, 1.5)
    assert free.capacity is None and sum(len(x["moves"]) for x in free.tree) > SLOT_CAP
    assert pc.SpecRun(lg, oracle.chess_from_fen(pc.START), SLOT_SIMS, SLOT_BS, 1.5, slot_cap=SLOT_CAP).capacity is None


def test_connect4_cases_reach_the_end_of_the_game(runs):
    late = pc.c4_board(pc.C4_LATE)
    assert 42 - late[0].count(".") >= 34 and puct_ref.C4Rules.moves(late)
    assert any(late[0][col] != "." for col in range(7))   # and a full column at the root
    assert any(b[0] != "." for b, _ in [pc.c4_board(pc.C4_COLS[2])])
    i = pc.C4_COLS.index(pc.C4_LATE)
    full = won = 0
    for case in pc.C4_CASES:
        term = [x for x in runs[case.name][i].tree if not x["moves"]]
        assert term, case.name
        full += sum((x["key"][0] | x["key"][1]).bit_count() == 42 for x in term)
        won += sum(oracle.check_win(*pc.C4.state(x["key"])) for x in term)
    assert full >= 1 and won >= 1, (full, won)


def test_the_limits_are_off_by_default():
    """puct_ref.search with the defaults, with limits out of reach and through puct_reuse_ref.search
    gives one answer; within reach it raises."""
    lg = pc.Logits(pc.Chess, "hash", 12)
    key = pc.Chess.key
    args = (65, 8, 1.5, lambda s: lg.value(key(s)), lambda node: lg.prior32(key(node.s)))
    for fen in (pc.START, pc.SLOT_FEN):
        s = oracle.chess_from_fen(fen)
        a = puct_ref.search(s, *args)
        assert a == puct_ref.search(s, *args, max_level=1000, slot_cap=1 << 30)
        assert a == puct_reuse_ref.search(puct_ref.Node(s), *args, rules=puct_ref.ChessRules)
        with pytest.raises(puct_ref.Capacity) as e:
            puct_ref.search(s, *args, max_level=2)
        assert e.value.kind == "depth"
        with pytest.raises(puct_ref.Capacity) as e:
            puct_ref.search(s, *args, slot_cap=500)
        assert e.value.kind == "slots"


PRIOR_MUTATIONS = ("transposed", "row", "all")   # the gather transposed / the leaf row off by one / softmax over the row
SEARCH_MUTATIONS = ("sign", "loss", "once")      # backup sign not alternating / virtual loss kept / repeats backed up once


def _rejects(check):
    try:
        check()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutation", PRIOR_MUTATIONS)
def test_check_priors_rejects_a_wrong_gather(runs, mutation):
    for case in pc.CASES:
        lg = case.logits()
        games = [i for i, s in enumerate(case.roots())
                 if _rejects(lambda: pc.check_priors(pc.SpecRun(lg, s, min(case.sims, 40), case.bs, case.c,
                                                                prior_mutation=mutation).tree, lg, case.name))]
        # every chess root; on Connect4 every root with a full column (with seven legal columns a
        # softmax over the row is the right one, and tie logits have no order to mirror)
        want = set(range(len(pc.CHESS_FENS))) if case.game is pc.Chess else {2, 3, 5}
        assert want <= set(games), (case.name, mutation, games)


@pytest.mark.parametrize("mutation", SEARCH_MUTATIONS)
def test_compare_trees_rejects_a_wrong_search(runs, mutation):
    """Where a mutation cannot show, that is asserted too: values 0 have no sign (the line cases and
    the zero-value case), and one leaf a flush is never pending twice."""
    for case in pc.CASES:
        lg = case.logits()
        hit = 0
        for s, want in zip(case.roots(), runs[case.name]):
            got = pc.SpecRun(lg, s, case.sims, case.bs, case.c, search_mutation=mutation)
            hit += _rejects(lambda: pc.compare_trees(got.tree, want.tree))
        if mutation == "once" and case.bs == 1:
            assert hit == 0 and all(r.repeats == 0 for r in runs[case.name])
        elif mutation == "sign" and case.zero_values:
            pass   # only a mate's or a win's -1 has a sign there
        else:
            assert hit >= 1, (case.name, mutation)
            if mutation != "once" and not case.zero_values:
                assert hit == len(case.roots()), (case.name, mutation, hit)
