"""The arena's routing kernels (arena.hip): the stable partition against its numpy
specification, and the row gather / scatter against torch indexing."""
import numpy as np
import pytest
import torch

from zeroclone_amd import _native
from zeroclone_amd.arena import route_ref

pytestmark = pytest.mark.gpu

WG = _native.ARENA_ROUTE_THREADS
SIZES = (1, 63, 64, 65, WG - 1, WG, WG + 1, 4096)


def keys(pattern: str, n: int) -> np.ndarray:
    if pattern == "zeros":
        return np.zeros(n, np.int32)
    if pattern == "ones":
        return np.ones(n, np.int32)
    if pattern == "alternating":
        return (np.arange(n) & 1).astype(np.int32)
    k = np.random.default_rng(n).integers(0, 2, n).astype(np.int32)
    if pattern == "junk":   # garbage above bit 0, the sign bit included
        k |= np.random.default_rng(n + 1).integers(-(1 << 30), 1 << 30, n).astype(np.int32) << 1
    return k


def route(key: np.ndarray):
    n = key.shape[0]
    d_key = torch.from_numpy(key).cuda()
    perm = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")   # two guard entries
    count = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    _native.arena_route(n, d_key.data_ptr(), perm.data_ptr(), count.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert perm[n:].tolist() == [-7, -7] and int(count[2]) == -7
    return perm[:n].cpu().numpy(), count[:2].cpu().numpy()


@pytest.mark.parametrize("pattern", ["zeros", "ones", "alternating", "random", "junk"])
def test_route_equals_route_ref(pattern):
    for n in SIZES:
        key = keys(pattern, n)
        perm, count = route(key)
        want_perm, want_count = route_ref(key)
        assert np.array_equal(count, want_count), (pattern, n)
        assert np.array_equal(perm, want_perm), (pattern, n)


def _sliced(n_elems: int, fill, odd: bool):
    """An int16 buffer of n_elems elements sliced from a larger one at element offset 1 (an odd
    2-byte offset: the base is 2-byte aligned and no more) or 0."""
    big = torch.empty(n_elems + 8, dtype=torch.int16, device="cuda")
    out = big[1:1 + n_elems] if odd else big[:n_elems]
    if isinstance(fill, torch.Tensor):
        out.copy_(fill)
    else:
        out.fill_(fill)
    assert out.data_ptr() % 4 == (2 if odd else 0)
    return out


N, GAME_ROWS, SENTINEL = 37, 8, -1234


def _perm(group: str) -> tuple[torch.Tensor, int]:
    key = {"none": np.ones(N, np.int32), "all": np.zeros(N, np.int32)}.get(group, keys("random", N))
    perm, count = route_ref(key)
    return torch.from_numpy(perm).cuda(), int(count[0])


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("row_bytes", [2, 6, 14, 28, 168, 2176, 4096, 8192])   # 28: the 4-byte access
def test_gather_and_scatter_equal_torch_indexing(row_bytes, odd):
    w = row_bytes // 2
    gen = torch.Generator().manual_seed(row_bytes)
    stream = torch.cuda.current_stream().cuda_stream
    for group in ("none", "all", "mixed"):
        perm, n_a = _perm(group)
        assert (n_a == 0, n_a == N) == (group == "none", group == "all")
        p = perm.long()
        for rows in (1, 3, GAME_ROWS):
            data = torch.randint(-30000, 30000, (N * GAME_ROWS * w,), dtype=torch.int16, generator=gen).cuda()
            src = _sliced(N * GAME_ROWS * w, data, odd)
            dst = _sliced(N * rows * w, SENTINEL, odd)
            _native.arena_gather(N, rows, GAME_ROWS, row_bytes, perm.data_ptr(), src.data_ptr(), dst.data_ptr(), stream)
            want = src.view(N, GAME_ROWS, w)[p][:, :rows]
            assert torch.equal(dst.view(N, rows, w), want), (group, rows)
            # the inverse, into a destination full of sentinels
            back = _sliced(N * GAME_ROWS * w, SENTINEL, odd)
            _native.arena_scatter(N, rows, GAME_ROWS, row_bytes, perm.data_ptr(), dst.data_ptr(), back.data_ptr(),
                                  stream)
            b = back.view(N, GAME_ROWS, w)
            want_back = torch.full_like(b, SENTINEL)
            want_back[p, :rows] = dst.view(N, rows, w)
            assert torch.equal(b, want_back), (group, rows)
            assert bool((b[:, rows:] == SENTINEL).all())                       # rows j >= rows untouched
            assert torch.equal(b[:, :rows], src.view(N, GAME_ROWS, w)[:, :rows])   # scatter o gather = identity


def test_copies_refuse_bad_arguments():
    t = torch.zeros(64, dtype=torch.int16, device="cuda")
    perm = torch.zeros(2, dtype=torch.int32, device="cuda")
    for rows, game_rows, row_bytes in ((0, 4, 8), (5, 4, 8), (1, 4, 7), (1, 4, 0)):
        with pytest.raises(ValueError):
            _native.arena_gather(2, rows, game_rows, row_bytes, perm.data_ptr(), t.data_ptr(), t.data_ptr())
    with pytest.raises(ValueError):
        _native.arena_scatter(2, 1, 4, 8, perm.data_ptr(), t.data_ptr() + 1, t.data_ptr())
