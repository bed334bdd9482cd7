"""The evaluation cache (csrc/evalcache.hip, zeroclone_amd/evalcache.py): the table and its two
kernels on random keys, the tower launches whose row count lives on the device, and the cached
callables against the plain ones — searches and self-play pools must return the same bits with
the cache as without it.  The argument checks at the end need no GPU."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

C4_PLANES, CHESS_PLANES = (2, 6, 7), (17, 8, 8)
STATS = ("probed", "hits", "inserts", "dropped")


# ---------------------------------------------------------------------------------------------
# helpers


def _bn(net):
    for m in net.modules():   # non-trivial folded BN, as tests/test_gpu_net.py:_net
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.1, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.1, 0.1)
    return net.eval()


def _value_model(in_planes, seed):
    from zeroclone_amd.nets import ValueNetwork
    torch.manual_seed(seed)
    return _bn(ValueNetwork(128, 2, in_planes=in_planes))


def _policy_model(game, seed):
    """PolicyValueNetwork cut to two residual blocks: Connect4 with the linear head (7 logits),
    chess with the convolutional head."""
    from zeroclone_amd.nets import PolicyValueNetwork
    torch.manual_seed(seed)
    net = PolicyValueNetwork(in_planes=2, board=(6, 7), n_logits=7) if game == "c4" else PolicyValueNetwork(head="conv")
    net.res = net.res[:2]
    return _bn(net)


class _Table:
    """A table in a buffer of the test's own, with 16 guard bytes on either side."""
    GUARD = 16

    def __init__(self, entries, key_bytes, logit_bytes):
        from zeroclone_amd import _native
        self.nat, self.sizes = _native, (entries, key_bytes, logit_bytes)
        self.bytes, self.sets = _native.evalcache_bytes(*self.sizes)
        self.buf = torch.zeros(self.bytes + 2 * self.GUARD, dtype=torch.uint8, device="cuda")
        self.buf[:self.GUARD] = 0xA5
        self.buf[-self.GUARD:] = 0x5A
        self.ptr = self.buf.data_ptr() + self.GUARD
        self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stats_t = torch.zeros(4, dtype=torch.int64, device="cuda")

    def guards_intact(self):
        return bool((self.buf[:self.GUARD] == 0xA5).all()) and bool((self.buf[-self.GUARD:] == 0x5A).all())

    def used_entries(self):
        """Entries whose meta word is not 0 (the layout of include/zeroclone.h: a 64-byte header,
        then one uint32 per entry)."""
        meta = self.buf[self.GUARD + 64: self.GUARD + 64 + 4 * 8 * self.sets].view(torch.int32)
        return int((meta != 0).sum())

    def stats(self):
        return dict(zip(STATS, (int(x) for x in self.stats_t.cpu())))

    def clear(self):
        self.nat.evalcache_clear(self.ptr, *self.sizes)

    def probe(self, keys, planes, out_v, out_l, rows=1, game_rows=1):
        """-> (missed rows in dense order, the dense planes of the misses)."""
        n_rows = keys.shape[0] // game_rows * rows
        dense = torch.full((n_rows, planes.shape[1]), -3.0, dtype=planes.dtype, device="cuda")
        miss = torch.full((n_rows,), -1, dtype=torch.int32, device="cuda")
        self.nat.evalcache_probe(self.ptr, *self.sizes, n_rows, rows, game_rows, keys.data_ptr(), planes.data_ptr(),
                                 planes.shape[1] * planes.element_size(), out_v.data_ptr(),
                                 out_l.data_ptr() if out_l is not None else 0, dense.data_ptr(), miss.data_ptr(),
                                 self.count.data_ptr(), self.stats_t.data_ptr())
        k = int(self.count.item())
        assert 0 <= k <= n_rows
        assert bool((miss[k:] == -1).all())
        self.miss = miss
        return miss[:k].cpu().numpy(), dense[:k]

    def commit(self, keys, dense_v, dense_l, out_v, out_l, rows=1, game_rows=1):
        n_rows = keys.shape[0] // game_rows * rows
        self.nat.evalcache_commit(self.ptr, *self.sizes, n_rows, rows, game_rows, keys.data_ptr(),
                                  self.miss.data_ptr(), self.count.data_ptr(), dense_v.data_ptr(),
                                  dense_l.data_ptr() if dense_l is not None else 0, out_v.data_ptr(),
                                  out_l.data_ptr() if out_l is not None else 0, self.stats_t.data_ptr())
        torch.cuda.synchronize()
        assert int(self.count.item()) == 0   # reset for the next flush

    def insert(self, keys, values, logits):
        """One flush of keys that the table does not hold: probe (all miss), commit."""
        n = keys.shape[0]
        planes = torch.zeros((n, 8), dtype=torch.float16, device="cuda")
        out_v = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        out_l = torch.full_like(logits, 0x5A) if logits is not None else None
        rows, _ = self.probe(keys, planes, out_v, out_l)
        idx = torch.from_numpy(rows.astype(np.int64)).cuda()
        self.commit(keys, values[idx].contiguous(), logits[idx].contiguous() if logits is not None else None,
                    out_v, out_l)
        return rows, out_v, out_l


def _random_keys(n, key_bytes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 62, 2 ** 62, (n, key_bytes // 8), generator=g, dtype=torch.int64).cuda()


def _payload(n, logit_bytes, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(n, generator=g, dtype=torch.float64).cuda()
    lg = torch.randint(0, 255, (n, logit_bytes), generator=g, dtype=torch.uint8).cuda() if logit_bytes else None
    return v, lg


# ---------------------------------------------------------------------------------------------
# 1. the table: no false hits


@gpu
@pytest.mark.parametrize("logit_bytes", [0, 16, 8192])
@pytest.mark.parametrize("key_bytes,plane_halfs", [(24, 84), (72, 1088)])
def test_table_hits_are_exact_and_misses_are_packed(key_bytes, plane_halfs, logit_bytes):
    """512 keys committed into 8192 entries, then probed mixed with 512 keys never inserted.
    plane_halfs: one row's planes — 84 fp16 (168 bytes: 8-byte accesses) and 1088 (2176: 16)."""
    t = _Table(8192, key_bytes, logit_bytes)
    n = 512
    keys = _random_keys(2 * n, key_bytes, seed=key_bytes + logit_bytes)
    assert len({tuple(r) for r in keys.cpu().tolist()}) == 2 * n
    vals, lgs = _payload(n, logit_bytes, seed=1)
    rows, out_v, out_l = t.insert(keys[:n].contiguous(), vals, lgs)
    assert sorted(rows.tolist()) == list(range(n))             # an empty table: every row missed once
    assert torch.equal(out_v, vals)                            # and the commit scattered every payload
    if logit_bytes:
        assert torch.equal(out_l, lgs)
    s = t.stats()
    assert s["probed"] == n and s["hits"] == 0 and s["inserts"] + s["dropped"] == n

    perm = torch.randperm(2 * n, generator=torch.Generator().manual_seed(5)).cuda()
    mixed = keys[perm].contiguous()
    planes = torch.randn((2 * n, plane_halfs), generator=torch.Generator().manual_seed(6)).half().cuda()
    out_v = torch.full((2 * n,), -7.0, dtype=torch.float64, device="cuda")
    out_l = torch.full((2 * n, logit_bytes), 0x5A, dtype=torch.uint8, device="cuda") if logit_bytes else None
    missed, dense = t.probe(mixed, planes, out_v, out_l)
    assert len(set(missed.tolist())) == len(missed)            # each missed row once
    src = perm.cpu().numpy()                                   # row i holds key src[i]
    miss_set = set(missed.tolist())
    hit_rows = [i for i in range(2 * n) if i not in miss_set]
    assert all(src[i] < n for i in hit_rows)                   # no never-inserted key hits
    print(f"key {key_bytes} logits {logit_bytes}: {len(hit_rows)} of {n} inserted keys hit; {t.stats()}")
    assert len(hit_rows) >= 0.99 * n
    hi = torch.tensor(hit_rows, device="cuda")
    assert torch.equal(out_v[hi], vals[perm[hi]])              # bit-equal payloads
    mi = torch.from_numpy(missed.astype(np.int64)).cuda()
    assert bool((out_v[mi] == -7.0).all())                     # missed rows' outputs untouched
    if logit_bytes:
        assert torch.equal(out_l[hi], lgs[perm[hi]])
        assert bool((out_l[mi] == 0x5A).all())
    assert torch.equal(dense.view(torch.int16), planes[mi].view(torch.int16))
    s2 = t.stats()
    assert s2["probed"] == 3 * n and s2["hits"] == len(hit_rows)
    assert s["inserts"] >= len(hit_rows) and t.used_entries() == s["inserts"]
    assert t.guards_intact()


@gpu
def test_table_short_flush_probes_each_games_first_rows_only():
    """rows_per_game 3 of game_rows 8: rows 3..7 of every game take no part."""
    t = _Table(1024, 24, 0)
    games, gr, nb = 16, 8, 3
    keys = _random_keys(games * gr, 24, seed=9)
    planes = torch.randn((games * gr, 84), generator=torch.Generator().manual_seed(2)).half().cuda()
    out_v = torch.full((games * gr,), -7.0, dtype=torch.float64, device="cuda")
    missed, dense = t.probe(keys, planes, out_v, None, rows=nb, game_rows=gr)
    want = sorted(g * gr + j for g in range(games) for j in range(nb))
    assert sorted(missed.tolist()) == want
    mi = torch.from_numpy(missed.astype(np.int64)).cuda()
    assert torch.equal(dense.view(torch.int16), planes[mi].view(torch.int16))
    dv = torch.arange(len(want), dtype=torch.float64, device="cuda")
    t.commit(keys, dv, None, out_v, None, rows=nb, game_rows=gr)
    assert torch.equal(out_v[mi], dv)
    rest = torch.ones(games * gr, dtype=torch.bool, device="cuda")
    rest[mi] = False
    assert bool((out_v[rest] == -7.0).all())
    out2 = torch.full_like(out_v, -7.0)
    missed2, _ = t.probe(keys, planes, out2, None, rows=nb, game_rows=gr)
    assert len(missed2) == 0 and torch.equal(out2, out_v)
    assert t.stats() == {"probed": 2 * len(want), "hits": len(want), "inserts": len(want), "dropped": 0}


# ---------------------------------------------------------------------------------------------
# 2. the table: one set


@gpu
@pytest.mark.parametrize("key_bytes,logit_bytes", [(24, 16), (72, 8192)])
def test_one_set_holds_at_most_its_ways_and_stays_inside_its_block(key_bytes, logit_bytes):
    t = _Table(8, key_bytes, logit_bytes)
    assert t.sets == 1
    n = 64
    keys = _random_keys(n, key_bytes, seed=3)
    vals, lgs = _payload(n, logit_bytes, seed=4)
    for lo in range(0, n, 16):
        t.insert(keys[lo:lo + 16].contiguous(), vals[lo:lo + 16], lgs[lo:lo + 16])
    s = t.stats()
    assert s["inserts"] + s["dropped"] == n and s["inserts"] >= 8 and s["dropped"] >= 8
    planes = torch.zeros((n, 8), dtype=torch.float16, device="cuda")
    out_v = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    out_l = torch.full_like(lgs, 0x5A)
    missed, _ = t.probe(keys, planes, out_v, out_l)
    hit = sorted(set(range(n)) - set(missed.tolist()))
    print(f"one set: rows {hit} hit; {s}")
    assert 1 <= len(hit) <= 8 and t.used_entries() == 8
    hi = torch.tensor(hit, device="cuda")
    assert torch.equal(out_v[hi], vals[hi]) and torch.equal(out_l[hi], lgs[hi])   # exact on the full key
    assert t.guards_intact()
    t.count.zero_()   # the probe above is not committed

    # the same key twice in one launch (a leaf pending twice in a flush): one entry, one dropped insert
    t.clear()
    torch.cuda.synchronize()
    assert t.used_entries() == 0
    before = t.stats()
    twice = keys[[5, 5]].contiguous()
    rows, out_v2, out_l2 = t.insert(twice, vals[[5, 5]].contiguous(), lgs[[5, 5]].contiguous())
    assert sorted(rows.tolist()) == [0, 1]
    assert torch.equal(out_v2, vals[[5, 5]]) and torch.equal(out_l2, lgs[[5, 5]])   # both rows got their output
    after = t.stats()
    assert after["inserts"] - before["inserts"] == 1 and after["dropped"] - before["dropped"] >= 1
    assert t.used_entries() == 1
    out_v3 = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    out_l3 = torch.full_like(out_l2, 0x5A)
    missed, _ = t.probe(twice, planes[:2], out_v3, out_l3)
    assert len(missed) == 0 and torch.equal(out_v3, out_v2) and torch.equal(out_l3, out_l2)
    assert t.guards_intact()


# ---------------------------------------------------------------------------------------------
# 3. the counted tower


@gpu
@pytest.mark.parametrize("shape", [CHESS_PLANES, C4_PLANES])
def test_counted_tower_evaluates_the_rows_below_the_count_alone(shape):
    """Capacity 37 (two boards a workgroup on 8x8, three on 6x7: a ragged last tile): for every
    device count the rows below it get the plain launch's bits — values, activation, policy
    output — and the rows at or past it keep the sentinel (-1: no ReLU output, and as a whole row
    no row of logits)."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, MfmaValueNetwork
    c, h, w = shape
    n, hw = 37, h * w
    x = (torch.rand((n, c, h, w), generator=torch.Generator().manual_seed(c)) < 0.3).half().cuda()
    x[36] = x[0]
    vnet = MfmaValueNetwork(_value_model(c, seed=11), "cuda")
    pnet = MfmaPolicyValueNetwork(_policy_model("c4" if c == 2 else "chess", seed=12), "cuda")
    a_ref, v_ref = (t.clone() for t in vnet.tower(x, head=True))
    pv_ref, _ = pnet(x)
    pv_ref = pv_ref.clone()
    p_ref = pnet._pout[(n, hw)].clone()
    torch.cuda.synchronize()
    for ref in (a_ref, p_ref):   # the same row at position 0 and at position 36: the same bits
        assert torch.equal(ref[0].view(torch.int16), ref[36].view(torch.int16))
    assert v_ref[0].item() == v_ref[36].item() and pv_ref[0].item() == pv_ref[36].item()
    for k in (0, 1, 5, 37, 50, -1, -2 ** 31):   # a negative count is 0 (include/zeroclone.h)
        cnt = torch.tensor([k], dtype=torch.int32, device="cuda")
        kk = max(min(k, n), 0)
        _, a_buf, _, _, v_buf = vnet._buffers(n, hw)
        a_buf.fill_(-1.0)
        v_buf.fill_(-5.0)
        a, v = vnet.tower(x, head=True, count=cnt)
        assert a.data_ptr() == a_buf.data_ptr() and v.data_ptr() == v_buf.data_ptr()
        assert torch.equal(a[:kk].view(torch.int16), a_ref[:kk].view(torch.int16)), k
        assert torch.equal(v[:kk], v_ref[:kk]), k
        assert bool((a[kk:] == -1.0).all()) and bool((v[kk:] == -5.0).all()), k
        v_buf.fill_(-5.0)
        v = vnet(x, count=cnt)   # the value-only launch (no activation written)
        assert torch.equal(v[:kk], v_ref[:kk]) and bool((v[kk:] == -5.0).all()), k
        p_buf, pv_buf = pnet._pout[(n, hw)], pnet.tower._buffers(n, hw)[4]
        p_buf.fill_(-1.0)
        pv_buf.fill_(-5.0)
        pv, _ = pnet(x, count=cnt)
        assert torch.equal(p_buf[:kk].view(torch.int16), p_ref[:kk].view(torch.int16)), k
        assert torch.equal(pv[:kk], pv_ref[:kk]), k
        assert bool((p_buf[kk:] == -1.0).all()) and bool((pv[kk:] == -5.0).all()), k


# ---------------------------------------------------------------------------------------------
# 4. the searches: the cached callable against the plain one

N_GAMES, BS = 8, 8


def _c4_roots():
    import oracle
    from zeroclone_amd._native import c4_from_rows
    lines = [[], [3], [3, 3], [3, 3, 2, 4], [0, 1, 2], [6, 5, 4, 3], [3, 2, 3, 2], [1, 1, 5, 5, 4]]
    rows = []
    for cols in lines:
        b, t = "." * 42, 0
        for col in cols:
            b, t = oracle.play(b, t, col)
        rows.append(c4_from_rows(b, t))
    return torch.from_numpy(np.array(rows).view(np.int64).reshape(len(lines), 3).copy()).cuda()


FENS = ["rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1",
        "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",
        "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1",
        "r1bqkbnr/pppp1ppp/2n5/4p3/2B1P3/5Q2/PPPP1PPP/RNB1K1NR w KQkq - 2 3",
        "6k1/5ppp/8/8/8/8/5PPP/3R2K1 w - - 0 1"]


def _chess_roots():
    from zeroclone_amd._native import CHESS_STATE_DTYPE, chess_from_fen
    fens = (FENS + FENS)[:N_GAMES]
    a = np.array([chess_from_fen(f) for f in fens], CHESS_STATE_DTYPE)
    return torch.from_numpy(a.view(np.uint8).reshape(N_GAMES, 72).copy()).cuda()


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=N_GAMES, max_sims=128, max_batch=BS)
    yield e
    e.close()


def _outputs(search):
    torch.cuda.synchronize()
    return {k: getattr(search, k).clone() for k in ("move", "na", "stats", "values")}


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@gpu
@pytest.mark.parametrize("game", ["c4", "chess"])
@pytest.mark.parametrize("sims", [64, 60])   # 60: the last flush holds 4 of the 8 leaves (rows())
def test_value_search_with_the_cache_returns_the_plain_search(eng, game, sims):
    from zeroclone_amd.evalcache import CachedValue, EvalCache
    from zeroclone_amd.nets import MfmaValueNetwork
    from zeroclone_amd.valued import C4ValuedSearch, ChessValuedSearch, NetValue
    roots = _c4_roots() if game == "c4" else _chess_roots()
    net = MfmaValueNetwork(_value_model(2 if game == "c4" else 17, seed=21), "cuda")
    seeds = list(range(50, 50 + N_GAMES))
    out = []
    cache = EvalCache(1 << 14, 24 if game == "c4" else 72, 0)
    for fn in (NetValue(net), CachedValue(net, cache)):
        vs = (C4ValuedSearch if game == "c4" else ChessValuedSearch)(eng, N_GAMES, BS, leaves=True)
        eng.seed(0, seeds)
        vs.run(roots, sims, 1.4, fn)
        out.append(_outputs(vs))
    _same(out[0], out[1], (game, sims))
    s = cache.stats()
    print(f"{game} value search, {sims} sims: {s}")
    assert s["probed"] == N_GAMES * (8 * (sims // BS) + sims % BS) and s["hits"] + s["inserts"] + s["dropped"] == s["probed"]
    if game == "c4":
        assert s["hits"] > 0


@gpu
@pytest.mark.parametrize("game", ["c4", "chess", "chess_nhwc"])
def test_puct_search_with_the_cache_returns_the_plain_search(eng, game):
    """Connect4 with the linear head (its GEMM runs on the dense rows: a row's logits must not
    depend on its position in the batch), chess with the convolutional head in both plane
    layouts.  A second search from the same roots without root noise finds every row."""
    from zeroclone_amd.evalcache import CachedPolicy, EvalCache
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    from zeroclone_amd.valued import C4PuctSearch, ChessPuctSearch, PolicyNet
    c4 = game == "c4"
    roots = _c4_roots() if c4 else _chess_roots()
    net = MfmaPolicyValueNetwork(_policy_model("c4" if c4 else "chess", seed=22), "cuda")
    cache = EvalCache(1 << 14, 24 if c4 else 72, 14 if c4 else 8192)
    kw = {} if c4 else dict(planes_nhwc=game == "chess_nhwc")
    out = []
    for fn in (PolicyNet(net), CachedPolicy(net, cache)):
        ps = (C4PuctSearch if c4 else ChessPuctSearch)(eng, N_GAMES, BS, seed=3, leaves=True, **kw)
        ps.run(roots, 64, fn, temperature=1.0)
        o = _outputs(ps)
        o["prior"] = ps.prior.clone()
        out.append(o)
    _same(out[0], out[1], game)
    s = cache.stats()
    print(f"{game} PUCT search: {s}")
    if c4:
        assert s["hits"] > 0
    # the same roots again, no noise, twice: the second search evaluates nothing
    ps = (C4PuctSearch if c4 else ChessPuctSearch)(eng, N_GAMES, BS, dirichlet_eps=0.0, leaves=True, **kw)
    ps.run(roots, 64, CachedPolicy(net, cache))
    first, s1 = _outputs(ps), cache.stats()
    ps.run(roots, 64, CachedPolicy(net, cache))
    d = _delta(cache.stats(), s1)
    _same(first, _outputs(ps), (game, "again"))
    assert d["inserts"] == 0 and d["dropped"] == 0 and d["hits"] == d["probed"] > 0, d


@gpu
def test_cached_value_search_replays_from_a_graph(eng):
    """capture() + two replay()s of the cached search (60 simulations: the short last flush is in
    the graph) equal two uncaptured runs of the plain search on the continuing game streams."""
    from zeroclone_amd.evalcache import CachedValue, EvalCache
    from zeroclone_amd.nets import MfmaValueNetwork
    from zeroclone_amd.valued import C4ValuedSearch, NetValue
    roots = _c4_roots()
    net = MfmaValueNetwork(_value_model(2, seed=23), "cuda")
    seeds = list(range(70, 70 + N_GAMES))
    vs = C4ValuedSearch(eng, N_GAMES, BS, leaves=True)
    eng.seed(0, seeds)
    want = []
    for _ in range(2):
        vs.run(roots, 60, 1.4, NetValue(net))
        want.append(_outputs(vs))
    cache = EvalCache(1 << 14, 24, 0)
    vc = C4ValuedSearch(eng, N_GAMES, BS, leaves=True)
    g = vc.capture(roots, 60, 1.4, CachedValue(net, cache))
    eng.seed(0, seeds)
    for i in range(2):
        g.replay()
        _same(want[i], _outputs(vc), ("replay", i))
    assert cache.stats()["hits"] > 0


@gpu
def test_cached_puct_search_replays_from_a_graph(eng):
    from zeroclone_amd.evalcache import CachedPolicy, EvalCache
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    from zeroclone_amd.valued import ChessPuctSearch, PolicyNet
    roots = _chess_roots()
    net = MfmaPolicyValueNetwork(_policy_model("chess", seed=24), "cuda")
    ps = ChessPuctSearch(eng, N_GAMES, BS, seed=5, leaves=True, planes_nhwc=True)
    want = []
    for _ in range(2):   # the search number moves the root noise and the sample on
        ps.run(roots, 64, PolicyNet(net), temperature=1.0)
        want.append(_outputs(ps))
    cache = EvalCache(1 << 14, 72, 8192)
    pc = ChessPuctSearch(eng, N_GAMES, BS, seed=5, leaves=True, planes_nhwc=True)
    g = pc.capture(roots, 64, CachedPolicy(net, cache), temperature=1.0)
    for i in range(2):
        g.replay()
        _same(want[i], _outputs(pc), ("replay", i))
    s = cache.stats()
    assert s["hits"] > 0 and s["probed"] > 0


# ---------------------------------------------------------------------------------------------
# 5. the pools


def _pool_state(pool):
    torch.cuda.synchronize()
    t = pool.traj
    names = ["hist", "hmoves", "slot", "ctl", "pool", "labels", "pool_moves", "games"]
    if t.policy_width is not None:
        names += ["slot_pi", "slot_off", "slot_base", "pctl", "pool_pi", "pool_first", "pool_count"]
    st = {"traj." + k: getattr(t, k).clone() for k in names}
    for k in ("roots", "moves", "results", "totals"):
        st[k] = getattr(pool, k).clone()
    return st


def _pool(kind, eval_cache, sims=64, **kw):
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, MfmaValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay
    if kind == "c4_value":
        return C4SelfPlay(N_GAMES, sims, batch_size=BS, seed=31, net=MfmaValueNetwork(_value_model(2, seed=32), "cuda"),
                          eval_cache=eval_cache, **kw)
    if kind.startswith("c4_puct"):
        return C4SelfPlay(N_GAMES, sims, batch_size=BS, seed=33, temperature=1.0, record_policy=True,
                          puct_net=MfmaPolicyValueNetwork(_policy_model("c4", seed=34), "cuda"),
                          reuse_tree=kind == "c4_puct_reuse", eval_cache=eval_cache, **kw)
    return ChessSelfPlay(N_GAMES, sims, batch_size=BS, seed=35, temperature=1.0, puct_streams=2,
                         puct_net=MfmaPolicyValueNetwork(_policy_model("chess", seed=36), "cuda"),
                         eval_cache=eval_cache, **kw)


@gpu
@pytest.mark.parametrize("kind,steps", [("c4_value", 12), ("c4_puct", 12), ("c4_puct_reuse", 12), ("chess_puct", 4)])
def test_pool_with_the_cache_plays_the_pool_without_it(kind, steps):
    """The trajectories in progress and finished (positions, labels, moves, visit counts), the
    games' states and the results after `steps` moves; the chess pool searches in two parts on
    two streams, each with a table of its own."""
    states = []
    for entries in (0, 1 << 16):
        pool = _pool(kind, entries)
        for _ in range(steps):
            pool.step()
        pool.check()
        states.append(_pool_state(pool))
        if entries:
            s = pool.eval_cache_stats()
            print(f"{kind}: {s}")
            assert s["hits"] > 0 and len(pool._caches) == (2 if kind == "chess_puct" else 1)
        else:
            with pytest.raises(ValueError):
                pool.eval_cache_stats()
        pool.close()
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), (kind, k)


@gpu
def test_set_network_empties_the_cache():
    """After set_network the pool plays what a fresh pool built with the new weights plays from
    the same state, and its counters move as the fresh pool's do: its table was empty.  65
    simulations: the roots flush and eight full ones, so every probed row is a pending leaf of
    the search at hand and the two pools probe the same rows."""
    from zeroclone_amd import learner
    from zeroclone_amd.selfplay import C4SelfPlay
    noiseless = dict(puct_args=dict(dirichlet_eps=0.0))   # a fresh pool's search numbers start again
    a = _pool("c4_puct", 1 << 16, sims=65, **noiseless)
    for _ in range(3):
        a.step()
    model2 = _policy_model("c4", seed=77)
    a.set_network(model2)
    a.temperature = 0.0
    torch.cuda.synchronize()
    assert all(int((c.table[64:64 + 4 * 8 * c.sets].view(torch.int32) != 0).sum()) == 0 for c in a._caches)
    s0 = a.eval_cache_stats()
    assert s0["inserts"] > 0
    b = C4SelfPlay(N_GAMES, 65, batch_size=BS, seed=33, temperature=0.0, record_policy=True,
                   puct_net=learner.inference_form(model2, a.dev), eval_cache=1 << 16, **noiseless)
    b.adopt(a)
    for _ in range(3):
        a.step()
        b.step()
    sa, sb = _pool_state(a), _pool_state(b)
    for k in ("roots", "moves", "results", "traj.hist", "traj.hmoves", "traj.slot", "traj.slot_pi", "traj.slot_off"):
        assert torch.equal(sa[k], sb[k]), k
    assert _delta(a.eval_cache_stats(), s0) == b.eval_cache_stats()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------
# 6. the argument checks (no GPU)


def test_eval_cache_refuses_bad_sizes():
    from zeroclone_amd.evalcache import EvalCache
    for entries in (0, -8):
        with pytest.raises(ValueError):
            EvalCache(entries, 24)
    for key_bytes in (20, 0, 7):
        with pytest.raises(ValueError):
            EvalCache(64, key_bytes)
    with pytest.raises(ValueError):
        EvalCache(64, 24, 7)
    with pytest.raises(ValueError):
        EvalCache(64, 24, device="cpu")


def test_cached_callables_refuse_torch_modules_and_missing_leaves():
    from zeroclone_amd.evalcache import CachedPolicy, CachedValue, EvalCache
    from zeroclone_amd.nets import (FoldedValueNetwork, MfmaPolicyValueNetwork, MfmaValueNetwork, PolicyValueNetwork,
                                    ValueNetwork)
    with pytest.raises(ValueError, match="MfmaValueNetwork"):
        CachedValue(FoldedValueNetwork(ValueNetwork(128, 1, in_planes=2)), EvalCache(64, 24))
    with pytest.raises(ValueError, match="MfmaPolicyValueNetwork"):
        CachedPolicy(PolicyValueNetwork(blocks=1), EvalCache(64, 72, 8192))

    class Value(MfmaValueNetwork):        # the type alone: no device behind it
        def __init__(self):
            pass

    class Policy(MfmaPolicyValueNetwork):
        conv_head, fused = True, True

        def __init__(self):
            pass

    planes = torch.zeros((16, 2, 6, 7), dtype=torch.float16)
    fn = CachedValue(Value(), EvalCache(64, 24))
    with pytest.raises(ValueError, match="leaves=True"):
        fn(None, planes, None)
    with pytest.raises(ValueError, match="leaves=True"):
        fn.rows(planes, 2, 8, 3, torch.zeros(16, dtype=torch.float64))
    with pytest.raises(ValueError, match="leaves=True"):
        CachedPolicy(Policy(), EvalCache(64, 72, 8192))(None, planes, None)
    with pytest.raises(ValueError, match="logits"):
        CachedPolicy(Policy(), EvalCache(64, 72, 14))
    with pytest.raises(ValueError, match="logits"):
        CachedValue(Value(), EvalCache(64, 24, 14))


def test_pools_refuse_what_the_cache_cannot_serve():
    from zeroclone_amd.arena import C4Arena, ChessArena
    from zeroclone_amd.selfplay import C4SelfPlay
    with pytest.raises(ValueError, match="eval_cache"):
        C4Arena(8, 64, net_a=object(), net_b=object(), eval_cache=1 << 10)
    with pytest.raises(ValueError, match="eval_cache"):
        ChessArena(8, 64, puct_net_a=object(), puct_net_b=object(), eval_cache=1 << 10)
    with pytest.raises(ValueError, match="eval_cache"):
        C4SelfPlay(8, 64, eval_cache=-1)
