"""Arena pools: two networks play each other on the device (scripts/evaluate.py at pool scale).

The reference gates a new network by `evaluate_pair` (scripts/evaluate.py:42-52): it builds
`Engine(cfg, value_functions=[latest, other])`, searches every move with `values[state.turn]`,
plays `games // 2` games with the new network moving first and the rest with it moving second,
and returns `(wins + 0.5 * draws) / games`.  `C4Arena` / `ChessArena` play those games as the
self-play pools play theirs — the same search kernels, recorder, quota and refill — with two
networks instead of one:

* Colours go by game number (start order).  In odd-numbered games network A is values[0] (it
  moves first), in even-numbered games values[1]: of games 0..N-1, N // 2 have A moving first
  and N - N // 2 second, evaluate_pair's split.
* Before each search every slot gets a key, turn(root) ^ (game number is even): 0 = network A
  is to move at the root, 1 = network B (idle slots: 0).  As in the reference, the network of
  the side to move at the root evaluates every leaf of that search.
* zc_arena_route_async partitions the slots by key; each flush's planes are gathered into that
  order, A runs on the first group and B on the second, and the outputs are scattered back
  (valued.RoutedValue / RoutedPolicy).  The search kernels see one callable, as in self-play.

The group size is data: after the first refill the side to move no longer follows slot order,
and how many slots hold which side changes every step.  The networks' batch shapes are host
values, so each step reads one int32 back (d_count[0]) and a step cannot be captured into a
graph.

With eval_cache= / eval_merge= the arena takes another path (evalcache.RoutedCachedValue /
RoutedCachedPolicy over a RoutedEvalCache): the keys go to the evaluation cache's routed flush
as they are, whose probe picks each row's table and dense list by its game's key — a table per
network, never a shared entry — and whose counted towers take the two group sizes from the
device.  There is no partition, no gather, no scatter and no host read: such an arena's step
can be captured (`capture_step()`), and it plays the games the plain arena plays, bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _native, valued
from .selfplay import C4SelfPlay, ChessSelfPlay, _check_mfma, simulate_games


def route_ref(key) -> tuple[np.ndarray, np.ndarray]:
    """zc_arena_route_async's specification: (perm, counts) of int32 keys — the indices whose
    key has bit 0 clear in ascending order, then those with it set in ascending order; counts =
    the two group sizes.  The key's other bits are ignored."""
    bit = np.asarray(key).astype(np.int64) & 1
    zeros, ones = np.flatnonzero(bit == 0), np.flatnonzero(bit == 1)
    return (np.concatenate([zeros, ones]).astype(np.int32),
            np.asarray([zeros.size, ones.size], dtype=np.int32))


@dataclass(frozen=True)
class ArenaResult:
    """Network A's record: (wins, draws, losses) in the games it moved first and in those it
    moved second."""
    first: tuple[int, int, int]
    second: tuple[int, int, int]

    @property
    def games(self) -> int:
        return sum(self.first) + sum(self.second)

    @property
    def score(self) -> float:
        """(wins + 0.5 * draws) / games over both colours: evaluate_pair's return value (its
        weighted mean of the two colours' win rates is this sum over all games)."""
        return (self.first[0] + self.second[0] + 0.5 * (self.first[1] + self.second[1])) / self.games

    @classmethod
    def tally(cls, results, game_numbers=None) -> "ArenaResult":
        """From the games' results (Engine._evaluate: +1 = the side with turn 0 won, -1 = the
        other side, 0 = a draw) by game number (default 0..len-1): A moved first in the
        odd-numbered games, where +1 is its win, and second in the even ones, where -1 is."""
        res = [int(r) for r in results]
        nos = range(len(res)) if game_numbers is None else [int(g) for g in game_numbers]
        rec = {True: [0, 0, 0], False: [0, 0, 0]}
        for g, r in zip(nos, res):
            if r not in (-1, 0, 1):
                raise ValueError(f"game {g}: result {r} is not one of -1, 0, +1")
            a_first = bool(g & 1)
            rec[a_first][1 - (r if a_first else -r)] += 1   # +1 for A: a win, 0: a draw, -1: a loss
        return cls(tuple(rec[True]), tuple(rec[False]))


class _ArenaPool:
    """What the two arenas add to their self-play pool (they subclass it): the two-network
    arguments and their refusals, the per-step route, `play()`, `set_networks()`.

    With openings= (the pool's book of openings) games 2k and 2k + 1 start from row k % N of the
    book: the colours still go by game number, so every opening is played once with network A as
    the side with turn 0 and once with network B.  An opening at an odd ply is fine: the route's
    key takes the root's turn, and `ArenaResult.tally` reads +1 as the side with turn 0."""

    _openings_share = 2

    def __init__(self, games: int, sims: int, *args, net_a=None, net_b=None, puct_net_a=None, puct_net_b=None,
                 temperature: float = 0.0, dirichlet_eps: float = 0.0, c_puct: float = 1.5,
                 dirichlet_alpha: float = 0.3, **kw):
        """net_a=, net_b=: the value search with two value networks; puct_net_a=, puct_net_b=:
        the PUCT search with two policy + value networks, by default without root noise and at
        temperature 0 (a gate measures the networks, not the exploration).  eval_cache=N /
        eval_merge=True (MFMA networks): an evaluation cache per network, N // 2 entries each,
        routed on the device (the module's last paragraph).  The pool's other arguments are its
        own.  The refusals come before the engine: they need no GPU."""
        value, puct = (net_a, net_b), (puct_net_a, puct_net_b)
        has_value, has_puct = any(x is not None for x in value), any(x is not None for x in puct)
        if has_value == has_puct or None in (value if has_value else puct):
            raise ValueError("an arena needs two networks of one search: net_a= and net_b=, or puct_net_a= and "
                             "puct_net_b=")
        if kw.get("reuse_tree"):
            raise ValueError("an arena keeps no tree between searches: a kept subtree would carry the opponent "
                             "network's values (reuse_tree)")
        if kw.get("record_policy"):
            raise ValueError("an arena records no policy targets (record_policy)")
        if kw.get("streams", 1) > 1 or kw.get("puct_streams", 1) > 1:
            raise ValueError("an arena searches on one stream (streams / puct_streams > 1): the two groups are not "
                             "contiguous game ranges")
        if kw.get("record", True) is not True:
            raise ValueError("an arena tells the colours by the recorder's game numbers (record=False)")
        if "net" in kw or "puct_net" in kw:
            raise ValueError("an arena takes net_a= / net_b= or puct_net_a= / puct_net_b=, not net= / puct_net=")
        if None not in puct:
            if bool(getattr(puct_net_a, "conv_head", False)) != bool(getattr(puct_net_b, "conv_head", False)):
                raise ValueError("the two PUCT networks must take the planes in one layout (conv_head)")
            kw["puct_args"] = dict(c_puct=c_puct, dirichlet_alpha=dirichlet_alpha, dirichlet_eps=dirichlet_eps)
        self._nets = value if has_value else puct
        self._conv_head = bool(getattr(self._nets[0], "conv_head", False))
        self._cached = bool(kw.get("eval_cache") or kw.get("eval_merge"))
        if self._cached:
            _check_mfma(value, puct, whose="both networks")
        self._counted = None   # the routed cache's (steps, mixed steps) on the device
        super().__init__(games, sims, *args, net=net_a, puct_net=puct_net_a, temperature=temperature, **kw)
        self._steps = self._mixed_steps = 0   # on the host: the plain arena's
        self.key = torch.zeros(games, dtype=torch.int32, device=self.dev)
        if self._cached:
            self.routed = self.value_fn if self.vs is not None else self.net_fn   # _callables below
            self.routed.set_route(self.key)
            self._counted = torch.zeros(2, dtype=torch.int64, device=self.dev)
            return
        if self.vs is not None:
            self._wrap = valued.NetValue
            self.value_fn = self.routed = valued.RoutedValue(valued.NetValue(net_a), valued.NetValue(net_b))
        else:
            self._wrap = valued.PolicyNet
            self.net_fn = self.routed = valued.RoutedPolicy(valued.PolicyNet(puct_net_a), valued.PolicyNet(puct_net_b))
        self._n_a = None   # the group size the networks' buffers were last allocated for
        self.perm = torch.zeros(games, dtype=torch.int32, device=self.dev)
        self.count = torch.zeros(2, dtype=torch.int32, device=self.dev)

    def _callables(self, net, k: int, puct: bool):
        """With eval_cache / eval_merge the search's callable is the routed cached one over both
        networks and a RoutedEvalCache: a table of max(eval_cache // 2, ways) entries per network
        (eval_cache = 0, eval_merge alone: no tables), both empty.  set_networks comes here again:
        the tables are kept where the logits row still fits them, emptied, and the counters go on
        counting."""
        if not self._cached:
            return super()._callables(net, k, puct)
        from . import evalcache
        key_bytes, logit_bytes, entries = self._cache_shape(self._nets[0], puct, 2)
        if not self._caches or self._caches[0].logit_bytes != logit_bytes:
            self._caches = [evalcache.RoutedEvalCache(entries, key_bytes, logit_bytes, self.dev, merge=self.eval_merge)]
        cache = self._caches[0]
        cache.clear()
        return (evalcache.RoutedCachedPolicy if puct else evalcache.RoutedCachedValue)(*self._nets, cache)

    def _inference_pair(self, model_a, model_b) -> tuple:
        """set_networks' two models as the searches evaluate them, or the refusal of a pair that is
        not of the arena's search and layout.  Needs no GPU unless a trained model is converted."""
        from . import learner, nets
        puct = self.ps is not None
        pair = []
        for m in (model_a, model_b):
            is_puct = isinstance(m, (nets.PolicyValueNetwork, nets.MfmaPolicyValueNetwork,
                                     learner.FoldedPolicyValueNetwork))
            is_value = isinstance(m, (nets.ValueNetwork, nets.MfmaValueNetwork, nets.FoldedValueNetwork))
            if (is_puct or is_value) and is_puct != puct:
                raise ValueError("this arena was built for the " + ("PUCT search: it takes two policy + value "
                                 "networks" if puct else "value search: it takes two value networks"))
            head = getattr(m, "conv_head", getattr(m, "head_kind", "linear") == "conv")
            if puct and bool(head) != self._conv_head:
                raise ValueError("the arena's search hands over the planes in the layout of the networks it was "
                                 "built with (conv_head): the new networks must take the same")
            pair.append(m)
        trained = (nets.ValueNetwork, nets.PolicyValueNetwork)
        return tuple(learner.inference_form(m, self.dev) if isinstance(m, trained) else m for m in pair)

    def set_networks(self, model_a, model_b):
        """Play model_a (network A) against model_b from the next step() on: the gate's hand-over
        (learner.full_training_run(gate=)).  Trained modules (`nets.ValueNetwork` /
        `nets.PolicyValueNetwork`) go through learner.inference_form; networks already in their
        inference form are taken as they are.  Both routed callables are replaced — on the plain
        path with their buffers, which the next route allocates for its group sizes — and both
        evaluation caches are emptied: an entry of an old network must never serve a new one.  A
        pair of another search (value / PUCT) or another conv_head than the arena was built with
        is refused.  A step graph captured before keeps the old weights, as `set_network`'s."""
        pair = self._inference_pair(model_a, model_b)
        puct = self.ps is not None
        if self._cached:
            _check_mfma(() if puct else pair, pair if puct else (), whose="both networks")
        self._nets = pair
        if self._cached:
            self.routed = self._callables(pair[0], 1, puct)   # both tables emptied
            self.routed.set_route(self.key)
        else:
            self.routed = (valued.RoutedPolicy if puct else valued.RoutedValue)(*(self._wrap(n) for n in pair))
            self._n_a = None
        if puct:
            self.net_fn = self.routed
        else:
            self.value_fn = self.routed

    def set_network(self, model):
        raise ValueError("an arena plays two networks: set_networks(model_a, model_b)")

    @property
    def steps(self) -> int:
        """Searches so far.  With the routed cache the count lives on the device: reading it
        synchronises (a step does not)."""
        return self._steps + (int(self._counted[0]) if self._counted is not None else 0)

    @property
    def mixed_steps(self) -> int:
        """The searches in which both networks had games (`steps`' note applies)."""
        return self._mixed_steps + (int(self._counted[1]) if self._counted is not None else 0)

    def eval_cache_stats(self, by_network: bool = False):
        """The pools' counters, summed over the two networks' tables; by_network=True: the pair
        (network A's, network B's).  Synchronises."""
        if not self._caches:
            raise ValueError("this pool was built without eval_cache or eval_merge")
        a, b = self._caches[0].stats()
        return (a, b) if by_network else {k: a[k] + b[k] for k in a}

    def _route(self):
        """key -> the routed cache's flush as it is; or -> partition -> the routed callable's
        group sizes: one small device read."""
        gno = self.traj.slot[:, 1]
        torch.where(gno >= 0, self._turn() ^ ((gno & 1) ^ 1), torch.zeros_like(gno), out=self.key)
        if self._cached:
            self.routed.set_route(self.key)
            n_b = self.key.sum()
            self._counted[0] += 1
            self._counted[1] += (n_b > 0) & (n_b < self.G)
            return
        _native.arena_route(self.G, self.key.data_ptr(), self.perm.data_ptr(), self.count.data_ptr(),
                            torch.cuda.current_stream(self.dev).cuda_stream)
        n_a = int(self.count[0])
        if n_a != self._n_a:
            # the MFMA networks keep their buffers per batch size, for ever: a new pair of sizes
            # gets replicas (shared weights, no buffers yet) and the old ones' buffers go
            self.routed.fns = tuple(self._wrap(net.replica() if hasattr(net, "replica") else net)
                                    for net in self._nets)
            self._n_a = n_a
        self.routed.set_route(self.perm, n_a)
        self._steps += 1
        self._mixed_steps += 0 < n_a < self.G

    def step_search(self, stream: int | None = None) -> torch.Tensor:
        if stream is not None and stream != torch.cuda.current_stream(self.dev).cuda_stream:
            raise ValueError("an arena steps on torch's current stream (its networks run there)")
        self._route()
        return super().step_search(stream)

    def capture_step(self):
        """With the routed cache (eval_cache / eval_merge) the pool's capture: the step reads
        nothing back.  The warm-up before the capture runs the networks on whatever the search's
        buffers hold, so its probes are taken out again: the tables are emptied and the counters
        put back.  The plain arena refuses: its two groups' sizes are host values read back every
        step (the networks' batch shapes), so one captured step cannot stand for the next."""
        if not self._cached:
            raise ValueError("an arena step cannot be captured without eval_cache or eval_merge: the two "
                             "networks' group sizes change every step and are read back from the device")
        cache = self._caches[0]
        counters = cache.counters.clone()
        g = super().capture_step()
        cache.clear()
        cache.counters.copy_(counters)
        return g

    def play(self, total_games: int, max_steps: int | None = None) -> ArenaResult:
        """evaluate_pair's games: `total_games` games under simulate_games' quota (games 0 ..
        total_games - 1 in start order, N // 2 of them with network A moving first), tallied
        on the host from the finished games' numbers and results.  The games stay in
        `last_batch`."""
        simulate_games(self, total_games, max_steps=max_steps)
        g = self.last_batch.games[:, [0, 2]].cpu().tolist()
        return ArenaResult.tally([r for _, r in g], [no for no, _ in g])


class C4Arena(_ArenaPool, C4SelfPlay):
    """Two networks play Connect4 against each other: `C4SelfPlay` with net_a= / net_b= (value
    search) or puct_net_a= / puct_net_b= (PUCT); `play(n).score` is evaluate_pair's win rate
    of network A.  step() only; run() / run_pooled() refuse as for every network mode."""

    def _turn(self) -> torch.Tensor:
        return (self.roots[:, 2] & 1).to(torch.int32)


class ChessArena(_ArenaPool, ChessSelfPlay):
    """Two networks play chess against each other: `ChessSelfPlay` with net_a= / net_b= or
    puct_net_a= / puct_net_b=."""

    def _turn(self) -> torch.Tensor:
        return self.roots[:, 64].to(torch.int32) & 1
