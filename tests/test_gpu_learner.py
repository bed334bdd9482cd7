"""The learner on the device: zc_train_batch_async and zc_train_loss_async against their
executable spec (tests/learner_ref.py) and the entry points they must agree with, the autograd
wrapper, and one training run handed back to a running pool.  The smallest shapes that cross
the kernels' boundaries: one row, a partial workgroup (5 = 4 + 1 rows), more than one workgroup
with a partial one (66, 67), a chess row with more than 64 legal moves (a lane holds two) and
one with none."""
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


# ---------------------------------------------------------------- the loss
ULP1 = 4.8e-7   # 4 ulp of 1.0 in fp32


def _loss_case(width, B, f16, scale, policy=True, seed=0):
    """Rows: 0 the longest legal list (70 moves: two to a lane / all 7 columns), 1 no legal move,
    every third a non-policy row, the last one with its legal logits near the dtype's largest
    finite value (the moves with a target all at one value, the others far below: the loss stays
    of order log n, and exp of an unshifted logit would overflow)."""
    g = np.random.default_rng(1000 * width + 10 * B + seed)
    stride = 7 if width == 7 else 256
    most = 7 if width == 7 else 70
    legal = np.zeros((B, stride), np.uint16)
    target = np.zeros((B, stride), np.float32)
    nl = g.integers(1, most + 1, B)
    nl[0] = most
    if B > 1:
        nl[1] = 0
    logits = (g.standard_normal((B, width)) * scale).astype(np.float32)
    for b in range(B):
        n = int(nl[b])
        if width == 7:
            legal[b, :n] = np.sort(g.choice(7, n, replace=False))
        else:
            sq = g.choice(4096, n, replace=False)
            legal[b, :n] = (sq // 64) | ((sq % 64) << 6) | (g.integers(0, 10, n) << 12)
        if policy and n and (b % 3 != 2 or b == B - 1):
            k = (g.integers(1, 33, n) * (g.random(n) < 0.7)).astype(np.int64)
            k[g.integers(0, n)] += 1
            target[b, :n] = k.astype(np.float32) / np.float32(k.sum())
    b = B - 1
    if nl[b]:
        big = 6.0e4 if f16 else 3.0e38
        at = learner_ref.logit_index(legal[b, :nl[b]], width)
        logits[b, at] = np.where(target[b, :nl[b]] > 0, big, big * 0.9)
    lt = torch.from_numpy(logits).to(torch.float16 if f16 else torch.float32)
    v = np.tanh(g.standard_normal(B)).astype(np.float32)
    z = g.integers(-1, 2, B).astype(np.float32)
    return dict(B=B, width=width, stride=stride, logits=lt.to(DEV), v=torch.from_numpy(v).to(DEV),
                z=torch.from_numpy(z).to(DEV), legal=torch.from_numpy(legal.view(np.int16)).to(DEV),
                n_legal=torch.from_numpy(nl.astype(np.int32)).to(DEV), target=torch.from_numpy(target).to(DEV),
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


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("width,B", [(7, 1), (7, 5), (7, 67), (4096, 3), (4096, 66)])
def test_loss_against_the_spec(width, B, f16):
    for scale, policy in ((1.0, True), (30.0, True), (1.0, False)):
        c = _loss_case(width, B, f16, scale, policy)
        h = c["np"]
        Lv, Lp, gv, gl = learner_ref.loss_ref(h["v"], h["logits"], h["z"], h["legal"], h["n_legal"], h["target"])
        loss, kgv, kgl = _kernel(c)
        tLv, tLp, tgv, tgl = _torch_fp32(c)
        err = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - b)))   # noqa: E731
        figures = {"Lv": (err(loss[0], Lv), err(tLv, Lv)), "Lp": (err(loss[1], Lp), err(tLp, Lp)),
                   "grad_v": (err(kgv, gv), err(tgv, gv))}
        if not f16:
            figures["grad_logits"] = (err(kgl.numpy(), gl), err(tgl, gl))
        print(f"width {width} B {B} f16 {f16} scale {scale} policy {policy}: Lp {Lp:.6g}",
              {k: (f"{a:.3g}", f"{t:.3g}") for k, (a, t) in figures.items()})
        for k, (mine, torchs) in figures.items():
            assert mine <= 2 * torchs + ULP1, (k, mine, torchs, scale, policy)
        if f16:   # against the fp64 gradient rounded to fp16: within one fp16 ulp
            want = gl.astype(np.float16)
            got = kgl.numpy()
            ulp = np.spacing(np.maximum(np.abs(want), np.abs(got)).astype(np.float16)).astype(np.float64)
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        # exact zeros off the policy rows' legal cells (the buffer held NaN)
        cells = np.zeros((B, width), bool)
        for b in range(B):
            n = int(h["n_legal"][b])
            if h["target"][b, :n].sum() > 0:
                cells[b, learner_ref.logit_index(h["legal"][b, :n], width)] = True
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
