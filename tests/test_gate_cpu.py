"""`learner.full_training_run(gate=)` with fakes: a pool whose games are finished at once, an
arena that returns scripted scores and a `train` stand-in that perturbs the weights.  No GPU."""
import copy

import pytest
import torch

from zeroclone_amd import learner
from zeroclone_amd.arena import ArenaResult
from zeroclone_amd.nets import ValueNetwork
from zeroclone_amd.selfplay import TrajBatch


class FakePool:
    """What full_training_run touches of a pool; every call goes into `calls`."""

    def __init__(self, calls):
        self.max_sims, self.sims, self.c, self.ps = 800, 0, 0.0, None
        self.calls, self.traj = calls, self

    def start(self, quota):
        self.calls.append(("start", quota))
        self.quota = quota

    def finished(self):
        return self.quota

    def step(self):
        raise AssertionError("the fake's games are finished at once")

    def take(self):
        self.calls.append(("take",))
        games = torch.zeros((self.quota, 5), dtype=torch.int64)   # the schedule's count of game records
        return TrajBatch(torch.zeros((6, 3), dtype=torch.int64), torch.zeros(6, dtype=torch.int32),
                         torch.zeros(6, dtype=torch.int16), games)

    def set_network(self, model):
        self.calls.append(("set_network", copy.deepcopy(model.state_dict())))


def result_with(score_halves: int, games: int) -> ArenaResult:
    """`games` games of which network A wins score_halves // 2 and draws score_halves % 2."""
    wins, draws = divmod(score_halves, 2)
    return ArenaResult((wins, draws, 0), (0, 0, games - wins - draws))


class FakeArena:
    def __init__(self, calls, results):
        self.calls, self.results = calls, list(results)

    def set_networks(self, model_a, model_b):
        self.calls.append(("set_networks", copy.deepcopy(model_a.state_dict()), copy.deepcopy(model_b.state_dict()),
                           model_a is not model_b))

    def play(self, games):
        self.calls.append(("play", games))
        return self.results.pop(0)


def make_train(calls):
    def fake_train(model, ts, epochs, lr, batch_size):
        calls.append(("train", len(ts)))
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.full_like(p, 0.125))
            for name, b in model.named_buffers():      # BatchNorm's running statistics move in training too
                if b.dtype.is_floating_point:
                    b.add_(0.5)
        return learner.TrainResult([0.0], 0.0)
    return fake_train


def same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def model_and_state():
    torch.manual_seed(4)
    model = ValueNetwork(8, 1, in_planes=2)
    return model, copy.deepcopy(model.state_dict())


def test_a_score_at_the_threshold_promotes_and_one_below_restores():
    """Cycle 0: 11 / 20 = 0.55 = the threshold: promoted.  Cycle 1: 10.5 / 20: not promoted, the
    weights go back to cycle 0's trained ones bit for bit.  Cycle 2: 1.0: promoted."""
    calls = []
    model, w0 = model_and_state()
    pool = FakePool(calls)
    results = [result_with(22, 20), result_with(21, 20), result_with(40, 20)]
    gate = learner.Gate(FakeArena(calls, results), games=20)
    assert gate.threshold == 0.55 and gate.history == []
    out = learner.full_training_run(pool, model, 3, train_fn=make_train(calls), gate=gate)
    assert len(out) == 3 and all(isinstance(r, learner.TrainResult) for r in out)
    assert [(c, p) for c, _, p in gate.history] == [(0, True), (1, False), (2, True)]
    assert [r for _, r, _ in gate.history] == results
    assert [c[0] for c in calls] == ["start", "take", "train", "set_networks", "play", "set_network",
                                     "start", "take", "train", "set_networks", "play",
                                     "start", "take", "train", "set_networks", "play", "set_network"]
    nets = [c for c in calls if c[0] == "set_networks"]
    promoted = [c[1] for c in calls if c[0] == "set_network"]
    # cycle 0: the trained weights against the initial ones, two modules
    assert not same(nets[0][1], w0) and same(nets[0][2], w0) and nets[0][3]
    assert same(promoted[0], nets[0][1])
    # cycle 1: trained from cycle 0's weights, against them; refused
    assert same(nets[1][2], nets[0][1]) and not same(nets[1][1], nets[0][1])
    # cycle 2 trains from the restored weights: its incumbent is cycle 0's network again
    assert same(nets[2][2], nets[0][1]) and same(nets[2][1], nets[1][1])
    assert same(promoted[1], nets[2][1]) and same(model.state_dict(), nets[2][1])
    assert all(c[1] == 20 for c in calls if c[0] == "play")


def test_below_the_threshold_nothing_changes():
    calls = []
    model, w0 = model_and_state()
    gate = learner.Gate(FakeArena(calls, [result_with(0, 8), result_with(8, 8)]), games=8, threshold=0.51)
    learner.full_training_run(FakePool(calls), model, 2, train_fn=make_train(calls), gate=gate)
    assert "set_network" not in [c[0] for c in calls]
    assert same(model.state_dict(), w0)                   # parameters and buffers, bit for bit
    assert [p for _, _, p in gate.history] == [False, False] and len(gate.history) == 2
    assert [r.score for _, r, _ in gate.history] == [0.0, 0.5]


def test_the_incumbent_is_a_copy_on_the_models_device_and_the_snapshot_precedes_training():
    calls = []
    model, w0 = model_and_state()
    gate = learner.Gate(FakeArena(calls, [result_with(16, 8)]), games=8)
    learner.full_training_run(FakePool(calls), model, 1, train_fn=make_train(calls), gate=gate)
    (_, trained, incumbent, distinct), = [c for c in calls if c[0] == "set_networks"]
    assert distinct and same(incumbent, w0) and same(trained, model.state_dict()) and not same(trained, w0)


def test_without_a_gate_the_loop_is_the_parents():
    calls = []
    model, _ = model_and_state()
    learner.full_training_run(FakePool(calls), model, 2, train_fn=make_train(calls))
    assert [c[0] for c in calls] == ["start", "take", "train", "set_network"] * 2
    with pytest.raises(TypeError):
        learner.Gate()                                     # arena and games are required
