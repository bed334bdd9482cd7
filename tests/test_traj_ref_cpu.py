"""tests/traj_ref.py, the trajectory recorder's model, checked without a GPU: its labels against
selfplay.dataset_labels, its refill against a restatement of simulate_games' loop, its multi-step
form against repeated single steps, a recorded game of tests/golden through it, and the scripted
tables' promise that no two rows or moves of a table are equal."""
import random

import numpy as np
import pytest

import traj_ref as tr
from traj_ref import TrajModel
from zeroclone_amd.selfplay import dataset_labels


def play(model, t, policy=False, single=True, reached=None, lo=0, hi=None):
    """Steps [lo, hi) of a scripted table through the model, one step at a time or at once."""
    hi = t["states"].shape[0] if hi is None else hi
    na = t.get("na") if policy else None
    rm = t.get("root_moves") if policy else None
    if not single:
        model.record_steps(t["states"][lo:hi], t["moves"][lo:hi], t["results"][lo:hi], hi - lo, reached,
                           None if na is None else na[lo:hi], None if rm is None else rm[lo:hi])
        return
    for k in range(lo, hi):
        res = [int(x) for x in t["results"][k]]
        nak = None if na is None else [na[k][g] if res[g] != tr.SKIP else () for g in range(model.n)]
        model.step([tuple(int(x) for x in r) for r in t["states"][k]], t["moves"][k], res, nak,
                   None if rm is None else rm[k], t["flags"][k] if "flags" in t else None,
                   t["rep"][k] if "rep" in t else None)


def state_of(m):
    keys = ["slot", "hist", "hmoves", "pool", "labels", "pool_moves", "games", "positions", "n_games", "next",
            "finished", "overflow"]
    if m.slot_cap is not None:
        keys += ["slot_pi", "slot_off", "pool_pi", "pool_first", "pool_count", "entries", "pi_overflow"]
    return {k: getattr(m, k) for k in keys}


def test_labels_of_every_length_and_result_equal_dataset_labels():
    for length in range(2, 46):
        for result in (-1, 0, 1):
            m = TrajModel(1, tr.init_row(1), 64, 64, 1)
            for p in range(1, length):
                m.record([tr.row_of(0, 0, p, 1)], [p], [result if p == length - 1 else tr.ONGOING])
            assert m.games[0] == (0, 0, result, 0, length)
            assert m.labels[:length] == dataset_labels(length, result).astype(int).tolist(), (length, result)
            assert m.pool[:length] == [tr.init_row(1)] + [tr.row_of(0, 0, p, 1) for p in range(1, length)]
            assert m.pool_moves[:length] == list(range(1, length)) + [-1]
            assert m.labels[length] is None and m.slot[0] == [1, 1]


def simulate_games(threads, total_games, lengths):
    """scripts/train.py:simulate_games with the engine reduced to game lengths: every unfinished
    game gets one move per round; each of the round's finished games starts a new game while fewer
    than total_games have started.  The reference lists a round's finished games in the iteration
    order of a set of game indices, which Python leaves open and which changes no game (every new
    game starts at the opening); the device keeps the new game in the finished game's slot and
    lists them in slot order, so does this loop.  Returns per round [(game, slot, refill or None)]."""
    first = min(total_games, threads)
    unfinished = set(range(first))
    final = [None] * first
    slot_of = {i: i for i in range(first)}
    plies = {i: 1 for i in range(first)}
    rounds = []
    while unfinished:
        for i in unfinished:
            plies[i] += 1
        finished_now = [i for i in sorted(unfinished, key=slot_of.get) if plies[i] == lengths[i]]
        events = []
        for idx in finished_now:
            unfinished.remove(idx)
            final[idx] = 0
            new = None
            if len(final) < total_games:
                final += [None]
                new = len(final) - 1
                unfinished.add(new)
                slot_of[new], plies[new] = slot_of[idx], 1
            events.append((idx, slot_of[idx], new))
        rounds.append(events)
    return rounds


@pytest.mark.parametrize("quota", [0, 1, 3, 5, 6, 7, 17])
def test_refill_and_quota_equal_simulate_games(quota):
    n = 6
    rng = random.Random(quota)
    lengths = [rng.choice((2, 2, 3, 4, 6)) for _ in range(max(quota, 1))]
    rounds = simulate_games(n, quota, lengths)
    m = TrajModel(n, tr.init_row(1), 8, 200, 40, quota=quota)
    assert [s[1] for s in m.slot] == [g if g < min(quota, n) else -1 for g in range(n)]
    for events in rounds:
        live = [(g, m.slot[g][1]) for g in range(n) if m.slot[g][1] >= 0]
        results = [tr.ONGOING] * n
        for g, game in live:
            if m.slot[g][0] + 1 == lengths[game]:
                results[g] = 0
        before = m.n_games
        states, out = m.record([tr.row_of(g, 0, m.slot[g][0], 1) for g in range(n)], [0] * n, results)
        got = [(rec[0], rec[1], m.slot[rec[1]][1] if m.slot[rec[1]][1] >= 0 else None)
               for rec in m.games[before:m.n_games]]
        assert got == events
        for g in range(n):
            if m.slot[g][1] < 0:
                assert out[g] == tr.IDLE or any(e[1] == g for e in events)
    assert all(s == [1, -1] for s in m.slot) and m.finished == quota and m.overflow == 0
    assert m.next == min(quota, n) + quota          # every finish counts, past the quota too
    states, out = m.record([(5,)] * n, [0] * n, [0] * n)
    assert states == [tr.init_row(1)] * n and out == [tr.IDLE] * n and m.finished == quota


def _random_case(seed):
    rng = random.Random(seed)
    n, steps = rng.randint(1, 9), rng.randint(1, 40)
    lengths = [[rng.choice((2, 2, 3, 5, 9)) for _ in range(rng.randint(0, 12))] for _ in range(n)]
    skip = [rng.choice((None, rng.randint(0, steps))) for _ in range(n)]
    stride = rng.choice((None, 7, 70))
    t = tr.scripted(n, steps, 8 * rng.choice((1, 3)), lengths, stride=stride, with_ids=bool(stride == 70),
                    skip_after=skip)
    return n, steps, t, stride


@pytest.mark.parametrize("seed", range(12))
def test_record_steps_equals_repeated_record(seed):
    n, steps, t, stride = _random_case(seed)
    words = t["states"].shape[2]
    for reached in (None, 0, -3, steps - 1, steps, steps + 5):
        kr = TrajModel.reached_steps(steps, reached)
        a, b, c = (TrajModel(n, tr.init_row(words), 64, 4000, 400, slot_cap=None if not stride else 300,
                             pi_pool_cap=20000) for _ in range(3))
        play(a, t, policy=bool(stride), single=True, hi=kr)
        frozen = {k: (None if v is None else v.copy()) for k, v in t.items()}
        play(b, t, policy=bool(stride), single=False, reached=reached)
        assert all(v is None or np.array_equal(v, frozen[k]) for k, v in t.items())   # tables not modified
        assert state_of(a) == state_of(b), (seed, reached)
        if stride:                                  # the two calls of a launch, policy first
            c.policy_record_steps(t["results"], t["na"], t["root_moves"], steps, reached)
            assert c.positions == 0 and c.slot == TrajModel(n, tr.init_row(words), 64, 1, 1).slot
            c.record_steps_after_policy(t["states"], t["moves"], t["results"], steps, reached)
            assert state_of(c) == state_of(a), (seed, reached)


def test_skip_leaves_a_slot_as_it_is():
    t = tr.scripted(2, 6, 8, [[4], [3, 3]], stride=7, skip_after=[2, None])
    m = TrajModel(2, tr.init_row(1), 8, 100, 10, slot_cap=40, pi_pool_cap=100)
    play(m, t, policy=True)
    assert m.slot[0] == [3, 0] and m.hist[0] == [tr.init_row(1), tr.row_of(0, 0, 1, 1), tr.row_of(0, 0, 2, 1)]
    assert len(m.slot_off[0]) == 3 and len(m.slot_pi[0]) == m.slot_off[0][2]
    assert [g[:3] for g in m.games[:2]] == [(1, 1, tr.result_of(1, 0)), (2, 1, tr.result_of(1, 1))]
    assert m.n_games == 2 and m.games[2] is None


def test_golden_selfplay_games_through_the_model(golden):
    """tests/golden/c4_selfplay.json holds the reference's games as moves and result (no fixture
    holds get_dataset's arrays): one slot per game, rows that name the move prefix."""
    games = golden("c4_selfplay.json")["games"]
    n, steps = len(games), max(len(g["moves"]) for g in games)
    m = TrajModel(n, (0, 0, 0), 43, sum(len(g["moves"]) + 1 for g in games), n, quota=n)
    rows = [[(0, 0, 0)] + [(hash(tuple(g["moves"][:p])) & (2 ** 62 - 1), p, p & 1)
                           for p in range(1, len(g["moves"]) + 1)] for g in games]
    for k in range(steps):
        st, mv, rs = [], [], []
        for g in games:
            live = k < len(g["moves"])
            st.append(rows[games.index(g)][k + 1] if live else (0, 0, 0))
            mv.append(g["moves"][k] if live else 0)
            rs.append((g["result"] if k + 1 == len(g["moves"]) else tr.ONGOING) if live else tr.ONGOING)
        m.record(st, mv, rs)
    assert m.finished == n and m.overflow == 0 and m.positions == m.pool_cap
    batch = m.take()
    assert [g[0] for g in batch["games"]] == list(range(n))
    for (game, slot, result, first, ln), g in zip(batch["games"], games):
        assert (slot, result, ln) == (game, g["result"], len(g["moves"]) + 1)
        assert batch["rows"][first:first + ln] == rows[game]
        assert batch["moves"][first:first + ln] == g["moves"] + [-1]
        assert batch["labels"][first:first + ln] == dataset_labels(ln, result).astype(int).tolist()


def test_chess_result_rule():
    for flags in range(8):
        for rep in (None, 0, 2, 3):
            for turn in (0, 1):
                want = turn * 2 - 1 if flags & 1 else (0 if (flags & 6 or rep == 3) else tr.ONGOING)
                assert tr.chess_result(turn, flags, rep) == want
    t = tr.scripted(5, 12, 72, [[2, 3, 4]] * 5, chess=True)
    m = TrajModel(5, tr.init_row(9), 8, 400, 40)
    want = t["results"].copy()
    for k in range(12):
        res = [77] * 5
        m.record([tuple(int(x) for x in r) for r in t["states"][k]], t["moves"][k], res, t["flags"][k], t["rep"][k])
        assert res == want[k].tolist()
    assert m.finished == 15 and {g[2] for g in m.games[:15]} == {-1, 0, 1}


def test_overflow_bits_of_the_model():
    t = tr.scripted(3, 4, 8, [[2, 3], [3], [6]])      # slot 2 reaches 5 positions and does not finish
    need = 2 + 3 + 3
    full = TrajModel(3, tr.init_row(1), 5, need, 3)
    play(full, t)
    assert full.overflow == 0 and full.positions == need and None not in full.pool
    short = TrajModel(3, tr.init_row(1), 5, need - 1, 3)
    play(short, t)
    assert short.overflow == tr.OV_POOL and short.positions == need and short.n_games == 3
    assert short.games[:2] == full.games[:2] and short.games[2] is None and short.pool[5:] == [None, None]
    assert short.slot == full.slot and short.hist == full.hist
    fewer = TrajModel(3, tr.init_row(1), 5, need, 2)
    play(fewer, t)
    assert fewer.overflow == tr.OV_POOL and fewer.pool[5:] == [None] * 3 and fewer.games == full.games[:2]
    tight = TrajModel(3, tr.init_row(1), 4, need, 3)
    play(tight, t)
    assert tight.overflow == tr.OV_MAXLEN and tight.unspecified == {2} and tight.slot[2] == [4, 2]
    assert tight.games == full.games and tight.hist[:2] == full.hist[:2] and tight.hist[2][:3] == full.hist[2][:3]
    exact = TrajModel(3, tr.init_row(1), 5, need, 3)
    play(exact, t)
    assert exact.overflow == 0 and exact.slot[2] == [5, 2]
    quota = TrajModel(3, tr.init_row(1), 5, need, 3, quota=3)
    quota.record_steps(t["states"], t["moves"], t["results"], 1)
    assert quota.overflow == tr.OV_QUOTA and quota.slot[0] == [1, -1]


def test_scripted_rows_and_moves_are_distinct():
    t = tr.scripted(65, 9, 24, [[2, 3, 2, 4]] * 65, stride=70, with_ids=True)
    words = t["states"].reshape(-1)
    assert len(set(words.tolist())) == words.size
    seen = {}
    for g in range(65):
        for j in range(6):
            for p in range(1, 9):
                assert seen.setdefault((tr.row_of(g, j, p, 3)), (g, j, p)) == (g, j, p)
    moves = t["moves"].reshape(-1).tolist()
    assert len(set(moves)) > 0.98 * len(moves) and min(moves) > 0
    for k in range(9):
        assert (t["na"][k].astype(bool).sum(1) == [tr.default_nnz(g, *_at(t, g, k), 70) for g in range(65)]).all()


def _at(t, g, k):
    """(game, position) slot g is at before step k of a table of games [2, 3, 2, 4]."""
    j, p = 0, 0
    for _ in range(k):
        p += 1
        if j < 4 and p + 1 == (2, 3, 2, 4)[j]:
            j, p = j + 1, 0
    return j, p
