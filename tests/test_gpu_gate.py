"""The gate in the training loop, end to end on the device: `learner.full_training_run(gate=)`
with a small value network, a Connect4 pool and a `C4Arena` over a book of openings.  A gate that
always promotes leaves the ungated run's games; one that never promotes leaves the weights and the
games of a run that never trained."""
import copy

import numpy as np
import pytest
import torch

from zeroclone_amd import learner
from zeroclone_amd.arena import C4Arena
from zeroclone_amd.nets import ValueNetwork
from zeroclone_amd.selfplay import C4SelfPlay

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CYCLES, GAMES, SIMS, BS = 2, 8, 16, 8


def c4_row(cols: str) -> list[int]:
    stones, height = [0, 0], [0] * 7
    for i, ch in enumerate(cols):
        c = int(ch)
        stones[i & 1] |= 1 << (7 * c + height[c])
        height[c] += 1
    return [stones[0], stones[1], len(cols) & 1]


BOOK = torch.tensor([c4_row("33"), c4_row("3"), c4_row("3342"), c4_row("2")], dtype=torch.int64)


def same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def run(threshold=None, trains=True):
    """Two cycles at games_cap 8 and sims_cap 16 from one seed.  Returns each cycle's self-play
    games, the model's state at the start of each cycle's training and at the end, and the gate."""
    torch.manual_seed(7)
    np.random.seed(7)
    model = ValueNetwork(8, 1, in_planes=2).to(DEV)          # the shape of tests/golden/ref_value_net_c8b1.pth
    pool = C4SelfPlay(GAMES, SIMS, batch_size=BS, seed=2, net=learner.inference_form(model, DEV))
    gate = None
    if threshold is not None:
        start = learner.inference_form(model, DEV)
        arena = C4Arena(GAMES, SIMS, batch_size=BS, seed=4, net_a=start, net_b=start, openings=BOOK)
        gate = learner.Gate(arena, games=GAMES, threshold=threshold)
    games, states = [], []

    def train_fn(m, ts, **kw):
        b = pool.last_batch
        games.append((b.rows.cpu(), b.labels.cpu(), b.moves.cpu(), b.games.cpu()))
        states.append(copy.deepcopy(m.state_dict()))
        # the shuffle from a generator of the cycle's own: building a network's inference form draws
        # from torch's global one (the folded convolutions' initialisers), and a gate builds more of them
        shuffle = torch.Generator().manual_seed(100 + len(games))
        return learner.train(m, ts, generator=shuffle, **kw) if trains else learner.TrainResult([0.0], 0.0)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True   # the convolutions' backward without atomics: runs repeat
    try:
        out = learner.full_training_run(pool, model, CYCLES, epochs=2, batch_size=32, games_cap=GAMES,
                                        sims_cap=SIMS, init_lr=1e-2, train_fn=train_fn, gate=gate)
    finally:
        torch.backends.cudnn.deterministic = was
    assert len(out) == CYCLES
    states.append(copy.deepcopy(model.state_dict()))
    pool.close()
    if gate is not None:
        gate.arena.close()
    return games, states, gate


_runs = {}


def cached(name, **kw):
    if name not in _runs:
        _runs[name] = run(**kw)
    return _runs[name]


def equal_games(x, y) -> bool:
    return all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(x, y))


def check_history(gate, promoted: bool):
    assert [(c, p) for c, _, p in gate.history] == [(0, promoted), (1, promoted)]
    assert all(r.games == GAMES and sum(r.first) == GAMES // 2 for _, r, _ in gate.history)


def test_a_gate_that_always_promotes_leaves_the_ungated_run():
    plain_games, plain_states, _ = cached("plain")
    games, states, gate = run(threshold=0.0)
    check_history(gate, True)
    assert len(games) == CYCLES and all(equal_games(x, y) for x, y in zip(games, plain_games))
    assert all(same(x, y) for x, y in zip(states, plain_states))
    assert not same(states[0], states[1]) and not same(states[1], states[2])     # it trained
    never = cached("never", trains=False)[0]
    assert not equal_games(plain_games[1], never[1]), "training left the second cycle's games as they were"


def test_a_gate_that_never_promotes_leaves_the_run_that_never_trained():
    never_games, never_states, _ = cached("never", trains=False)
    games, states, gate = run(threshold=1.01)
    check_history(gate, False)
    assert all(same(s, never_states[0]) for s in states)         # before each cycle and at the end: the initial weights
    assert all(equal_games(x, y) for x, y in zip(games, never_games)) and len(games) == CYCLES
    assert equal_games(games[0], cached("plain")[0][0])           # the first cycle is every run's
