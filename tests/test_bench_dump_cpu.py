"""bench.py's --dump-outputs bookkeeping and option surface, without a GPU: the launches'
per-step outputs (C4SelfPlay.run / run_pooled: a slot's moves of a launch are its first rows,
ZC_SLOT_SKIP after them) are laid out by the move's number since the first launch, whatever
share of the moves each launch played, and slots left short are played on by run()."""
import numpy as np
import torch


class _FakePool:
    """Plays fixed per-slot move sequences through launches of given per-slot move counts."""
    dev = torch.device("cpu")
    first_id = 100

    def __init__(self, moves, results, states):
        self.seq = (results, moves, states)
        self.at = np.zeros(moves.shape[0], np.int64)
        self.completed = []

    def launch(self, cap, counts):
        from zeroclone_amd import _native
        g = len(counts)
        r = np.full((cap, g), _native.ZC_SLOT_SKIP, np.int32)
        m = np.full((cap, g), -1, np.int16)
        s = np.zeros((cap, g, 3), np.int64)
        for i, n in enumerate(counts):
            for k in range(n):
                r[k, i], m[k, i], s[k, i] = (a[i, self.at[i]] for a in self.seq)
                self.at[i] += 1
        self._run_results, self._run_moves, self._run_states = (torch.from_numpy(x) for x in (r, m, s))

    def run(self, k):
        self.completed.append(k)
        self.launch(k, [k] * len(self.at))


def _sequences(g, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 7, (g, n)).astype(np.int16), rng.integers(-1, 3, (g, n)).astype(np.int32),
            rng.integers(0, 1 << 49, (g, n, 3)))


def test_dump_is_indexed_by_move_number_whatever_the_launches_played(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    g, n = 6, 7
    moves, results, states = _sequences(g, 40, 3)
    files = []
    for shares in ([[0, 1, 2, 4, 3, 2], [2, 10, 5, 3, 0, 7], [1, 0, 1, 0, 1, 0]],   # warm-up, timed, drain
                   [[4, 4, 0, 1, 3, 2], [10, 3, 9, 6, 2, 5], [0, 1, 1, 1, 0, 0]]):
        sp = _FakePool(moves, results, states)
        log = bench.MoveLog(torch.arange(g))
        for cap, counts in zip((4, 10, 1), shares):
            sp.launch(cap, counts)
            log.add(sp)
        played = log.played()
        assert list(played) == [sum(s[i] for s in shares) for i in range(g)]
        out = tmp_path / f"d{len(files)}"
        rep = bench.dump_outputs(sp, log, n, str(out))
        assert sp.completed == [n - int(played.min())] and rep["completed_untimed_moves"] == sp.completed[0]
        files.append({k: np.load(out / f"{k}.npy") for k in ("moves", "results", "states", "game_ids")})
    a, b = files
    assert a["moves"].dtype == a["results"].dtype == a["game_ids"].dtype == np.float32
    assert a["states"].dtype == np.float64
    assert np.array_equal(a["moves"], moves[:, :n]) and np.array_equal(a["results"], results[:, :n])
    assert np.array_equal(a["states"], states[:, :n].astype(np.float64))
    assert np.array_equal(a["states"].astype(np.int64), states[:, :n])   # 49-bit masks survive float64
    assert list(a["game_ids"]) == [100 + i for i in range(g)]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_sample_is_fixed_and_fits_the_size_limit():
    import bench
    every = bench.dump_slots(4096, 25, 0, "cpu")
    assert every.tolist() == list(range(4096))
    some = bench.dump_slots(4096, 5000, 0, "cpu")
    again = bench.dump_slots(4096, 5000, 0, "cpu")
    assert torch.equal(some, again) and some.tolist() == sorted(set(some.tolist()))
    assert 0 < some.numel() < 4096 and int(some.max()) < 4096
    assert some.numel() * 5000 * bench.DUMP_MOVE_BYTES + 4 * some.numel() <= 64 << 20
    assert bench.dump_slots(4096, 1 << 19, 0, "cpu").numel() * (1 << 19) * bench.DUMP_MOVE_BYTES <= 64 << 20


def test_plain_run_is_the_default():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
