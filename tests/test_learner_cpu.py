"""The learner without a GPU: the loss's executable spec against autograd, the replay sample,
`train` against the reference's own loop (tests/golden/train_value_c8b1.json) and
`full_training_run`'s schedule."""
import numpy as np
import pytest
import torch

import learner_ref
from zeroclone_amd import learner
from zeroclone_amd.learner import Minibatch, ReplaySet, TrainingSet
from zeroclone_amd.selfplay import ReplayBuffer, schedule_hyperparams


def _loss_case(seed, B, width, stride, n_legal, policy_rows, scale=1.0):
    """Random logits, legal lists of the given lengths (distinct logit indices) and targets on the
    rows of `policy_rows`."""
    g = np.random.default_rng(seed)
    legal = np.zeros((B, stride), np.uint16)
    target = np.zeros((B, stride), np.float32)
    for b in range(B):
        n = n_legal[b]
        if width == 7:
            legal[b, :n] = np.sort(g.choice(7, n, replace=False))
        else:
            sq = g.choice(4096, n, replace=False)
            legal[b, :n] = (sq // 64) | ((sq % 64) << 6) | (g.integers(0, 10, n) << 12)
        if b in policy_rows and n:
            # 64 visits over some of the moves: the fractions are dyadic and sum to exactly 1, where
            # (p - t) / P IS the gradient of Lp (in general it is (p * sum t - t) / P, and a visit
            # distribution rounded to fp32 sums to 1 only within an ulp or so)
            k = g.multinomial(64, g.dirichlet(np.ones(n))) if n > 1 else np.asarray([64])
            target[b, :n] = (k.astype(np.float32) / np.float32(k.sum()))
    return dict(v=np.tanh(g.normal(size=B)), z=g.integers(-1, 2, B).astype(np.float32),
                logits=g.normal(size=(B, width)) * scale, legal=legal, n_legal=np.asarray(n_legal, np.int32),
                target=target)


def _mb(c, width):
    return Minibatch(None, torch.from_numpy(c["z"]), torch.from_numpy(c["legal"].astype(np.int16)),
                     torch.from_numpy(c["n_legal"]), torch.from_numpy(c["target"]), torch.zeros(1, dtype=torch.int32),
                     width)


@pytest.mark.parametrize("width,stride,n_legal,policy_rows", [
    (7, 7, [7, 3, 0, 5, 1], {0, 1, 4}),            # row 2: no legal moves; row 3: no targets
    (7, 7, [4, 0, 7], set()),                      # P = 0
    (4096, 256, [20, 0, 130, 35, 1], {0, 2, 4}),   # more than 64 moves in a row
])
def test_loss_ref_matches_autograd_of_masked_log_softmax(width, stride, n_legal, policy_rows):
    c = _loss_case(11 + width, len(n_legal), width, stride, n_legal, policy_rows, scale=3.0)
    Lv, Lp, gv, gl = learner_ref.loss_ref(c["v"], c["logits"], c["z"], c["legal"], c["n_legal"], c["target"])
    v = torch.tensor(c["v"], dtype=torch.float64, requires_grad=True)
    x = torch.tensor(c["logits"], dtype=torch.float64, requires_grad=True)
    tv, tp = learner.loss_torch(v, x, _mb(c, width))
    (tv + tp).backward()
    assert abs(tv.item() - Lv) <= 1e-12 and abs(tp.item() - Lp) <= 1e-12
    np.testing.assert_allclose(v.grad.numpy(), gv, rtol=0, atol=1e-12)
    np.testing.assert_allclose(x.grad.numpy(), gl, rtol=0, atol=1e-12)
    if not policy_rows:
        assert Lp == 0.0 and not gl.any()
    # everything outside the policy rows' legal cells is exactly zero
    mask = np.zeros_like(gl, bool)
    for b in policy_rows:
        mask[b, learner_ref.logit_index(c["legal"][b, :n_legal[b]], width)] = True
    assert not gl[~mask].any() and not x.grad.numpy()[~mask].any()


def test_loss_torch_follows_the_headers_rules_for_hand_made_rows():
    """Where `loss_torch` once departed from zc_train_loss_async's definition (rows that
    `minibatch` never makes): a width-7 id above 6 is ignored, not read as column 6; a policy row
    is decided by the targets of its legal slots, not by the whole target row; n_legal outside
    [0, stride] is clamped."""
    c = learner_ref.hand_made_rule_rows()
    legal, target, nl = c["legal"], c["target"], c["n_legal"]
    Lv, Lp, gv, gl = learner_ref.loss_ref(c["v"], c["logits"], c["z"], legal, nl, target)
    v = torch.tensor(c["v"], dtype=torch.float64, requires_grad=True)
    x = torch.tensor(c["logits"], dtype=torch.float64, requires_grad=True)
    tv, tp = learner.loss_torch(v, x, _mb(c, 7))
    (tv + tp).backward()
    assert abs(tv.item() - Lv) <= 1e-12 and abs(tp.item() - Lp) <= 1e-12
    np.testing.assert_allclose(x.grad.numpy(), gl, rtol=0, atol=1e-12)
    np.testing.assert_allclose(v.grad.numpy(), gv, rtol=0, atol=1e-12)
    # the spec itself: rows 3, 5 and 6 are no policy rows, the ignored ids' columns get no gradient
    assert not gl[[3, 5, 6]].any() and gl[7].all() and gl[0, 6] != 0
    assert not gl[0, [0, 1, 3, 4]].any() and np.count_nonzero(gl[1]) == 2 and np.count_nonzero(gl[2]) == 4
    # by hand, row 0 alone: the softmax over columns 2, 5, 6 and the targets on them
    one = learner_ref.loss_ref(c["v"][:1], c["logits"][:1], c["z"][:1], legal[:1], nl[:1], target[:1])
    xs = c["logits"][0, [2, 5, 6]]
    logp = xs - np.log(np.exp(xs).sum())
    assert abs(one[1] + (np.asarray([0.25, 0.25, 0.5]) * logp).sum()) <= 1e-12


def test_loss_ref_value_only():
    c = _loss_case(5, 6, 7, 7, [7] * 6, set())
    Lv, Lp, gv, gl = learner_ref.loss_ref(c["v"], None, c["z"], None, None, None)
    v = torch.tensor(c["v"], dtype=torch.float64, requires_grad=True)
    tv, tp = learner.policy_value_loss(v, None, _mb(c, 7))
    tv.backward()
    assert abs(tv.item() - Lv) <= 1e-12 and tp.item() == 0.0 and Lp == 0.0 and gl is None
    np.testing.assert_allclose(v.grad.numpy(), gv, rtol=0, atol=1e-12)


def _c4_set(seed, n, policy=True):
    """Random (not necessarily reachable) Connect4 rows with labels and visit counts on playable
    columns."""
    g = np.random.default_rng(seed)
    rows = np.zeros((n, 3), np.int64)
    off, pi = [0], []
    for i in range(n):
        s = [0, 0]
        for c in range(7):
            for r in range(int(g.integers(0, 7))):
                s[int(g.integers(0, 2))] |= 1 << (7 * c + r)
        rows[i] = (s[0], s[1], int(g.integers(0, 2)))
        free = [c for c in range(7) if not ((s[0] | s[1]) >> (7 * c + 5)) & 1]
        ent = [c | (int(g.integers(1, 40)) << 16) for c in free if g.random() < 0.7] if i % 5 else []
        pi += ent
        off.append(len(pi))
    labels = torch.from_numpy(g.integers(-1, 2, n).astype(np.int32))
    ts = TrainingSet("c4", torch.from_numpy(rows), labels)
    if policy:
        ts.pi_off, ts.pi = torch.tensor(off, dtype=torch.int64), torch.tensor(pi, dtype=torch.int64).to(torch.int32)
    return ts


def _np(ts):
    return (ts.rows.numpy(), ts.labels.numpy(), None if ts.pi_off is None else ts.pi_off.numpy(),
            None if ts.pi is None else ts.pi.numpy())


def test_cpu_minibatch_is_the_spec():
    ts = _c4_set(3, 60)
    idx = torch.tensor([59, 7, 7, 0, 31, 30, 12, 58, 5])
    flip = torch.tensor([1, 0, 1, 0, 0, 1, 1, 0, 1], dtype=torch.bool)
    for mirror in (None, flip):
        mb = learner.minibatch(ts, idx, mirror)
        ref = learner_ref.batch_ref("c4", *_np(ts), idx.numpy(), None if mirror is None else mirror.numpy())
        np.testing.assert_array_equal(mb.planes.numpy(), ref["planes"])
        np.testing.assert_array_equal(mb.z.numpy(), ref["z"])
        np.testing.assert_array_equal(mb.legal.numpy().astype(np.uint16), ref["legal"])
        np.testing.assert_array_equal(mb.n_legal.numpy(), ref["n_legal"])
        np.testing.assert_array_equal(mb.target.numpy(), ref["target"])
        assert int(mb.status) == ref["status"] == 0
        mb.check()
    with pytest.raises(ValueError, match="mirror"):
        learner.minibatch(TrainingSet("chess", torch.zeros((2, 9), dtype=torch.int64), torch.zeros(2, dtype=torch.int32)),
                          torch.tensor([0]), torch.tensor([True]))


def test_cpu_minibatch_flags_an_illegal_entry():
    ts = _c4_set(4, 10)
    rows = ts.rows.clone()
    rows[1, 0] |= 0x3F << 14          # column 2 full
    rows[1, 1] &= ~(0x3F << 14)
    rows[1, 0] &= ~(0x3F << 28)
    rows[1, 1] &= ~(0x3F << 28)       # column 4 empty
    ts = TrainingSet("c4", rows, ts.labels, torch.tensor([0, 0, 2] + [2] * 8),
                     torch.tensor([2 | 5 << 16, 4 | 3 << 16], dtype=torch.int32))
    mb = learner.minibatch(ts, torch.tensor([1]))
    ref = learner_ref.batch_ref("c4", *_np(ts), [1])
    assert ref["status"] == 1 and int(mb.status) == 1
    np.testing.assert_array_equal(mb.target.numpy(), ref["target"])
    assert np.float32(3) / np.float32(8) in mb.target.numpy()
    with pytest.raises(RuntimeError, match="not legal"):
        mb.check()


def test_replay_set_draws_replay_buffers_rows():
    sets = [_c4_set(20 + k, n) for k, n in enumerate((50, 33, 41))]
    np.random.seed(99)
    buf, want = ReplayBuffer(), []
    for s in sets:
        want.append(buf.update(s.rows, s.labels))
    np.random.seed(99)
    rep = ReplaySet()
    for s, (rows, labels) in zip(sets, want):
        got = rep.update(s)
        assert torch.equal(got.rows, rows) and torch.equal(got.labels, labels)
        assert len(got) == len(rows) and got.pi_off[0] == 0 and got.pi_off[-1] == got.pi.numel()
        assert bool((got.pi_off[1:] >= got.pi_off[:-1]).all())
        # every row kept its own entries: the dense targets of the result = those of the sources
        allsets = TrainingSet.cat(sets)
        key = {tuple(r): i for i, r in enumerate(allsets.rows.tolist())}
        src = torch.tensor([key[tuple(r)] for r in got.rows.tolist()])
        a = learner.minibatch(got, torch.arange(len(got)))
        b = learner.minibatch(allsets, src)
        assert torch.equal(a.target, b.target) and torch.equal(a.legal, b.legal)
    # a private generator leaves numpy's global one alone
    np.random.seed(1)
    before = np.random.get_state()[1].copy()
    r2 = ReplaySet(seed=5)
    r2.update(sets[0])
    assert len(r2.update(sets[1])) == int(0.3 * 50) + 33
    assert (np.random.get_state()[1] == before).all()


def test_select_and_cat_keep_the_csr():
    ts = _c4_set(8, 25)
    idx = torch.tensor([24, 3, 3, 0, 10])
    sub = ts.select(idx)
    assert len(sub) == 5
    for j, i in enumerate(idx.tolist()):
        assert torch.equal(sub.pi[sub.pi_off[j]:sub.pi_off[j + 1]], ts.pi[ts.pi_off[i]:ts.pi_off[i + 1]])
    both = TrainingSet.cat([sub, ts])
    assert len(both) == 30 and torch.equal(both.pi, torch.cat([sub.pi, ts.pi]))
    assert TrainingSet.cat([ts, _c4_set(9, 4, policy=False)]).pi is None
    with pytest.raises(ValueError):
        TrainingSet.cat([ts, TrainingSet("chess", torch.zeros((1, 9), dtype=torch.int64), torch.zeros(1, dtype=torch.int32))])


def test_train_matches_the_references_loop(golden):
    """learner.train on the CPU against the reference's own `train` on the same 40 positions
    (tests/golden/gen_golden_train.py).  Tolerance: 10 x the spread the reference itself showed
    between a 1-thread and a 16-thread run, with assert_close's fp32 defaults as the floor; a
    wrong optimiser, label order or loss weighting is orders of magnitude beyond it."""
    from zeroclone_amd.nets import ValueNetwork
    g = golden("train_value_c8b1.json")
    cases = golden("chess_tensor.json")["cases"][:g["positions"]]
    rows = torch.from_numpy(np.stack([learner_ref.chess_row(c["state"]) for c in cases]))
    ts = TrainingSet("chess", rows, torch.tensor(g["labels"], dtype=torch.int32))
    # the decoded planes are the reference's state_to_tensor
    bits = np.stack([np.unpackbits(np.frombuffer(bytes.fromhex(c["bits"]), np.uint8))[:17 * 64] for c in cases])
    mb = learner.minibatch(ts, torch.arange(len(ts)))
    np.testing.assert_array_equal(mb.planes.numpy().reshape(len(ts), -1), bits.astype(np.float32))
    torch.manual_seed(g["seed"])
    model = ValueNetwork(8, 1)
    res = learner.train(model, ts, epochs=g["epochs"], lr=g["lr"], batch_size=g["batch_size"], shuffle=False,
                        device="cpu")
    rtol = max(10 * g["thread_rel_diff"], 1.3e-6)
    tol = dict(rtol=rtol, atol=1e-5)
    torch.testing.assert_close(torch.tensor(res.epoch_losses), torch.tensor(g["epoch_losses"]), **tol)
    torch.testing.assert_close(torch.tensor(res.reference_return), torch.tensor(g["returned"]), **tol)
    lin = model.head[2]
    torch.testing.assert_close(lin.weight.detach().reshape(-1), torch.tensor(g["head_weight"]), **tol)
    torch.testing.assert_close(lin.bias.detach().reshape(()), torch.tensor(g["head_bias"]), **tol)
    # the quirk: not the mean of the epoch averages
    assert abs(res.reference_return - float(np.mean(res.epoch_losses))) > 100 * rtol


def test_train_policy_network_on_cpu_learns_and_repeats():
    from zeroclone_amd.nets import PolicyValueNetwork
    ts = _c4_set(13, 96)
    out = []
    for _ in range(2):
        torch.manual_seed(3)
        model = PolicyValueNetwork(channels=8, blocks=1, in_planes=2, board=(6, 7), n_logits=7)
        g = torch.Generator().manual_seed(7)
        out.append(learner.train(model, ts, epochs=3, lr=3e-3, batch_size=32, generator=g, mirror=True, device="cpu"))
    assert out[0].epoch_losses == out[1].epoch_losses
    assert out[0].epoch_losses[-1] < out[0].epoch_losses[0]
    assert out[0].policy_losses[0] > 0


# `train` of the commit before the status of every batch was kept, on the setup above (8 CPU threads)
EPOCH_LOSSES_BEFORE = [2.979426066080729, 2.6508039633433023, 2.5597496032714844]


def _train_checking_the_last_batch_only(model, ts, epochs, lr, batch_size, generator):
    """`learner.train` as it stood (mirror=True, shuffle=True, CPU): the same calls in the same
    order, the status word of the epoch's last batch alone."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    n, losses = len(ts), []
    for _ in range(epochs):
        model.train()
        order = torch.randperm(n, generator=generator)
        running = torch.zeros((), dtype=torch.float64)
        for lo in range(0, n, batch_size):
            idx = order[lo:lo + batch_size]
            flip = torch.rand(idx.shape[0], generator=generator) < 0.5
            mb = learner.minibatch(ts, idx, flip)
            opt.zero_grad()
            v, logits = model(mb.planes)
            Lv, Lp = learner.policy_value_loss(v, logits, mb)
            loss = Lv + Lp
            loss.backward()
            opt.step()
            running = running + loss.detach().double() * idx.shape[0]
        mb.check()
        losses.append(float(running) / n)
    return losses


def test_train_on_a_clean_set_is_unchanged_by_keeping_every_status():
    """Exactly the losses of the loop that checked the last batch only, run here; and the values
    that loop gave when the change was made, within the spread that the number of CPU threads
    alone makes in them (1 thread: 2.9794263, 8 threads: 2.9794261: below 1e-7 relative)."""
    from zeroclone_amd.nets import PolicyValueNetwork
    ts = _c4_set(13, 96)
    net = lambda: PolicyValueNetwork(channels=8, blocks=1, in_planes=2, board=(6, 7), n_logits=7)  # noqa: E731
    torch.manual_seed(3)
    got = learner.train(net(), ts, epochs=3, lr=3e-3, batch_size=32, generator=torch.Generator().manual_seed(7),
                        mirror=True, device="cpu")
    torch.manual_seed(3)
    before = _train_checking_the_last_batch_only(net(), ts, 3, 3e-3, 32, torch.Generator().manual_seed(7))
    assert got.epoch_losses == before
    np.testing.assert_allclose(got.epoch_losses, EPOCH_LOSSES_BEFORE, rtol=1.3e-6, atol=0)


def _set_with_an_entry_on_a_full_column(n=64):
    """A clean set but for row 0, whose first entry names a full column."""
    ts = _c4_set(17, n)
    rows = ts.rows.clone()
    rows[0, 0] |= 0x3F << 14          # column 2 full
    rows[0, 1] &= ~(0x3F << 14)
    rows[0, 0] &= ~(0x3F << 28)
    rows[0, 1] &= ~(0x3F << 28)       # column 4 empty
    cnt = (ts.pi_off[1:] - ts.pi_off[:-1]).tolist()
    pi = torch.cat([torch.tensor([2 | 5 << 16, 4 | 3 << 16], dtype=torch.int32), ts.pi[cnt[0]:]])
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor([2] + cnt[1:]), 0)])
    return TrainingSet("c4", rows, ts.labels, off, pi)


def test_train_reports_an_illegal_entry_of_any_batch():
    """The status word of every batch of the epoch, not the last one's alone: the bad row is in the
    first of two batches."""
    from zeroclone_amd.nets import PolicyValueNetwork
    ts = _set_with_an_entry_on_a_full_column()
    assert int(learner.minibatch(ts, torch.arange(4)).status) == 1
    assert int(learner.minibatch(ts, torch.arange(32, 64)).status) == 0
    torch.manual_seed(3)
    model = PolicyValueNetwork(channels=8, blocks=1, in_planes=2, board=(6, 7), n_logits=7)
    with pytest.raises(RuntimeError, match="not legal"):
        learner.train(model, ts, epochs=1, lr=3e-3, batch_size=32, shuffle=False, device="cpu")
    good = ts.select(torch.arange(1, 64))
    learner.train(model, good, epochs=1, lr=3e-3, batch_size=32, shuffle=False, device="cpu")


class _StubPool:
    """What full_training_run touches of a pool."""

    def __init__(self, max_sims):
        self.max_sims, self.sims, self.c, self.ps = max_sims, 0, 0.0, None
        self.log, self.networks = [], []
        self.traj = self

    def start(self, quota):
        self.quota = quota

    def finished(self):
        return self.quota

    def step(self):
        raise AssertionError("the stub's games are finished at once")

    def take(self):
        self.log.append((self.quota, self.sims, self.c))
        n = 6
        from zeroclone_amd.selfplay import TrajBatch
        games = torch.zeros((self.quota, 5), dtype=torch.int64)
        return TrajBatch(torch.zeros((n, 3), dtype=torch.int64), torch.zeros(n, dtype=torch.int32),
                         torch.zeros(n, dtype=torch.int16), games)

    def set_network(self, model):
        self.networks.append(model)


def test_full_training_run_follows_the_schedule():
    pool, model, seen = _StubPool(max_sims=200), object(), []

    def fake_train(m, ts, epochs, lr, batch_size):
        seen.append((m, len(ts), epochs, lr, batch_size))
        return learner.TrainResult([0.0], 0.0)
    res = learner.full_training_run(pool, model, 3, epochs=2, batch_size=64, train_fn=fake_train)
    hp = [schedule_hyperparams(c) for c in range(3)]
    assert pool.log == [(h["games"], h["simulations"], h["c_puct"]) for h in hp]
    assert [s[3] for s in seen] == [h["lr"] for h in hp]
    assert [s[1] for s in seen] == [6, int(0.3 * 6) + 6, int(0.3 * 12) + 6]   # the replay sample grows
    assert all(s[0] is model and s[2] == 2 and s[4] == 64 for s in seen)
    assert pool.networks == [model] * 3 and len(res) == 3
    with pytest.raises(ValueError, match="max_sims"):
        learner.full_training_run(_StubPool(max_sims=110), model, 3, train_fn=fake_train)
