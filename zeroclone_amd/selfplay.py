"""Device-resident self-play, its trajectories, and the multi-GPU trajectory exchange.

`C4SelfPlay` / `ChessSelfPlay` are the batched form of scripts/train.py:simulate_games
(:151-170) + Engine.play_mcts_parallel (engine/engine.py:131-138): G games live on one GPU;
one `step()` searches every game, plays the chosen moves and evaluates them
(Engine.play_move/_evaluate) on the device; both are `_SelfPlayPool` with the game's launches
filled in.  Game slot g of rank r is global slot r*G + g
and draws from its own CPython MT19937 stream seeded seed + global slot id, so per-game
results do not depend on the number of GPUs.

Trajectories never leave the device while games are played (`Trajectories`,
zc_traj_record_async): every position is appended to its slot's game in HBM; a finished game
is labelled exactly as Engine.get_dataset (engine.py:60-89) labels it and copied to a
device pool, and its slot restarts from the opening (or goes idle once simulate_games'
quota of games has started); with `openings=` a pool restarts its slots from a book of openings
instead, by game number (zc_traj_openings_async, `openings_from_games`).  `take()` returns the
pool's games in start order as device tensors; `gather_positions` all-gathers every rank's
positions (counts first, then a padded payload) over torch.distributed — RCCL over xGMI on the
GPUs, gloo on CPU — the one collective of the scale-out path; `ReplayBuffer`
is scripts/train.py:_update_replay (:27-50) over device tensors.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import os

import numpy as np
import torch

from . import _native, valued

ONGOING = _native.ZC_C4_ONGOING
IDLE = _native.ZC_SLOT_IDLE
_UNLIMITED = 1 << 62


def dataset_labels(n_states: int, result: int) -> np.ndarray:
    """Engine.get_dataset's labels for one finished history of n_states positions
    (initial ... terminal): factor starts at 0 (draw) or -1, alternates sign, and the
    per-game list is appended REVERSED (engine.py:72-81)."""
    factor = 0 if result == 0 else -1
    entry = []
    for _ in range(n_states):
        entry.append(factor)
        factor = -factor
    return np.asarray(list(reversed(entry)), dtype=np.float32)


def planes(positions: np.ndarray) -> np.ndarray:
    """Compact rows -> c4_backend.state_to_tensor planes [n, 2, 6, 7] (side to move first)."""
    n = positions.shape[0]
    out = np.zeros((n, 2, 6, 7), np.float32)
    s0 = positions[:, 0].astype(np.uint64)
    s1 = positions[:, 1].astype(np.uint64)
    turn = (positions[:, 2] & 1).astype(np.int64)
    for r in range(6):
        for c in range(7):
            bit = np.uint64(1) << np.uint64(7 * c + (5 - r))
            x = (s0 & bit) != 0
            o = (s1 & bit) != 0
            out[:, 0, r, c] = np.where(turn == 0, x, o)
            out[:, 1, r, c] = np.where(turn == 0, o, x)
    return out


@dataclass
class TrajBatch:
    """Finished games taken from a `Trajectories` pool, in start order (device tensors).

    rows   [n, row_bytes // 8] int64  positions (zc_c4_state / zc_chess_state records)
    labels [n] int32                  Engine.get_dataset label of each position
    moves  [n] int16                  move played from it (-1 at a game's last position)
    games  [k, 5] int64               game number, slot, result, first row, positions

    With the root visit counts recorded (`Trajectories(policy_width=...)`; None otherwise):
    pi_off [n + 1] int64              row i owns the entries pi[pi_off[i]:pi_off[i + 1]]
    pi     [total] int32              move id | visit count << 16 (the uint32 entries), one per
                                      root move with Na > 0 in the root's move-list order; none
                                      at a game's last position (never searched)
    """
    rows: torch.Tensor
    labels: torch.Tensor
    moves: torch.Tensor
    games: torch.Tensor
    pi_off: torch.Tensor | None = None
    pi: torch.Tensor | None = None

    def results(self) -> list[int]:
        return [int(r) for r in self.games[:, 2].cpu().tolist()]

    def policy_targets(self, width: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """Dense policy targets [n, width] (zc_traj_policy_dense_async): N(a) / sum N per row,
        zeros elsewhere (a game's last position: all zeros).  width 7: index = column;
        width 4096: index = from * 64 + to, the order of the chess PUCT network's logits."""
        if self.pi is None:
            raise ValueError("no visit counts were recorded (record_policy=True / Trajectories(policy_width=...))")
        if dtype not in (torch.float32, torch.float16):
            raise ValueError("dtype must be torch.float32 or torch.float16")
        n = self.rows.shape[0]
        out = torch.empty((n, int(width)), dtype=dtype, device=self.rows.device)
        count = (self.pi_off[1:] - self.pi_off[:-1]).to(torch.int32)
        _native.check(_native.lib().zc_traj_policy_dense_async(
            n, ctypes.c_void_p(self.pi_off.data_ptr()), ctypes.c_void_p(count.data_ptr()),
            ctypes.c_void_p(self.pi.data_ptr()), int(width),
            _native.ZC_F16 if dtype == torch.float16 else _native.ZC_F32, ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)))
        return out


class Trajectories:
    """Per-slot game histories and the pool of finished games, all in HBM (zc_traj_record_async).

    `max_len` positions per game (Connect4: 43), room for `games_cap` finished games and
    `pool_cap` positions until the next `take()`.

    `policy_width` (7: Connect4, 4096: chess) also records every search's root visit counts,
    sparse (zc_traj_policy_*): `record_policy()` after the search, the commit inside
    `record()`; the fused launches' staged counts go through `record_steps(na=...)`.  `pi_slot_cap` entries per slot's game (default: every move of every position
    visited) and `pi_pool_cap` pooled entries until the next `take()`."""

    PI_STRIDE = {7: 7, 4096: _native.CHESS_MAX_MOVES}   # policy_width -> moves per root (d_out_root_na's row)

    def __init__(self, n_slots: int, init_row: torch.Tensor, max_len: int, games_cap: int, pool_cap: int,
                 device: torch.device, policy_width: int | None = None, pi_slot_cap: int | None = None,
                 pi_pool_cap: int | None = None):
        init = init_row.reshape(-1).contiguous().view(torch.uint8)
        if init.numel() % 8:
            raise ValueError("row size must be a multiple of 8 bytes")
        if policy_width is not None and policy_width not in self.PI_STRIDE:
            raise ValueError(f"policy_width must be 7 or 4096 (got {policy_width})")
        self.n, self.W, self.max_len, self.dev = n_slots, init.numel() // 8, max_len, device
        self.policy_width = policy_width
        if policy_width is not None:
            self.pi_stride = self.PI_STRIDE[policy_width]
            self.pi_slot_cap = int(pi_slot_cap) if pi_slot_cap is not None else (max_len - 1) * self.pi_stride
            self.pi_pool_cap = int(pi_pool_cap) if pi_pool_cap is not None else pool_cap * min(self.pi_stride, 32)
            self.slot_pi = torch.zeros((n_slots, self.pi_slot_cap), dtype=torch.int32, device=device)
            self.slot_off = torch.zeros((n_slots, max_len + 1), dtype=torch.int32, device=device)
            self.slot_base = torch.zeros(n_slots, dtype=torch.int64, device=device)
            self.pctl = torch.zeros(4, dtype=torch.int64, device=device)
        self.init = init.view(torch.int64).to(device).clone()
        self.hist = torch.zeros((n_slots, max_len, self.W), dtype=torch.int64, device=device)
        self.hmoves = torch.zeros((n_slots, max_len), dtype=torch.int16, device=device)
        self.slot = torch.zeros((n_slots, 4), dtype=torch.int32, device=device)
        self.ctl = torch.zeros(8, dtype=torch.int64, device=device)
        self._alloc_pool(games_cap, pool_cap)
        self.start(None)

    def _alloc_pool(self, games_cap: int, pool_cap: int):
        if getattr(self, "pinned", False):
            # a captured step graph has this pool's pointers baked into its record kernel:
            # replacing the buffers would leave the graph writing into freed memory
            raise RuntimeError(f"the trajectory pool ({self.games_cap} games, {self.pool_cap} positions) is held by "
                               f"a captured step graph and cannot grow to ({games_cap}, {pool_cap}); construct the "
                               "self-play pool with a larger games_cap before capture_step()")
        self.games_cap, self.pool_cap = int(games_cap), int(pool_cap)
        self.pool = torch.zeros((self.pool_cap, self.W), dtype=torch.int64, device=self.dev)
        self.labels = torch.zeros(self.pool_cap, dtype=torch.int32, device=self.dev)
        self.pool_moves = torch.zeros(self.pool_cap, dtype=torch.int16, device=self.dev)
        self.games = torch.zeros((self.games_cap, 4), dtype=torch.int64, device=self.dev)
        b = _native.TrajBuffers()
        b.row_bytes, b.max_len, b.pool_cap, b.games_cap = 8 * self.W, self.max_len, self.pool_cap, self.games_cap
        for f, t in (("d_hist", self.hist), ("d_hmoves", self.hmoves), ("d_slot", self.slot), ("d_pool", self.pool),
                     ("d_labels", self.labels), ("d_pool_moves", self.pool_moves), ("d_games", self.games),
                     ("d_ctl", self.ctl), ("d_init", self.init)):
            setattr(b, f, t.data_ptr())
        self._buf = b
        if self.policy_width is not None:
            self._alloc_pi(self.pi_pool_cap)

    def _alloc_pi(self, pi_pool_cap: int):
        """The pooled policy entries and each pooled position's (first, count); the per-slot
        history keeps its buffers."""
        self.pi_pool_cap = int(pi_pool_cap)
        self.pool_pi = torch.zeros(self.pi_pool_cap, dtype=torch.int32, device=self.dev)
        self.pool_first = torch.zeros(self.pool_cap, dtype=torch.int64, device=self.dev)
        self.pool_count = torch.zeros(self.pool_cap, dtype=torch.int32, device=self.dev)
        q = _native.TrajPolicyBuffers()
        q.slot_cap, q.pi_pool_cap = self.pi_slot_cap, self.pi_pool_cap
        for f, t in (("d_slot_pi", self.slot_pi), ("d_slot_off", self.slot_off), ("d_slot_base", self.slot_base),
                     ("d_pool_pi", self.pool_pi), ("d_pool_first", self.pool_first),
                     ("d_pool_count", self.pool_count), ("d_pctl", self.pctl)):
            setattr(q, f, t.data_ptr())
        self._pol = q

    def _grow_pool(self, games_cap: int, pool_cap: int, pi_pool_cap: int | None = None):
        """A larger pool holding the positions and game records (and policy entries) reserved so far."""
        ctl = self.ctl.cpu().tolist()
        npos, ngames = int(ctl[_native.ZC_TRAJ_POSITIONS]), int(ctl[_native.ZC_TRAJ_GAMES])
        old = (self.pool, self.labels, self.pool_moves, self.games)
        if self.policy_width is not None:
            nent = min(int(self.pctl[_native.ZC_TRAJ_PI_ENTRIES]), self.pi_pool_cap)
            old_pi = (self.pool_pi, self.pool_first, self.pool_count)
            self.pi_pool_cap = max(self.pi_pool_cap, int(pi_pool_cap or 0))
        self._alloc_pool(games_cap, pool_cap)
        self.pool[:npos] = old[0][:npos]
        self.labels[:npos] = old[1][:npos]
        self.pool_moves[:npos] = old[2][:npos]
        self.games[:ngames] = old[3][:ngames]
        if self.policy_width is not None:
            self.pool_pi[:nent] = old_pi[0][:nent]
            self.pool_first[:npos] = old_pi[1][:npos]
            self.pool_count[:npos] = old_pi[2][:npos]

    def ensure_room(self):
        """Grow the pool (on demand, keeping its contents) so that the next step cannot
        overflow it: a slot's game that finishes at that step has at most its current
        history length + 1 positions, so the worst case is known before the step — far less
        than quota x max_len.  One small device read; simulate_games calls it per step.
        The policy entries likewise: the live slots' current entry fill plus one row of moves each."""
        act = self.slot[:, 1] >= 0
        need = [(self.slot[:, 0].to(torch.int64) + 1)[act].sum(), act.sum().to(torch.int64)]
        ctl = [self.ctl[_native.ZC_TRAJ_POSITIONS], self.ctl[_native.ZC_TRAJ_GAMES]]
        if self.policy_width is not None:
            fill = self.slot_off.gather(1, (self.slot[:, :1].to(torch.int64) - 1).clamp(0, self.max_len))[:, 0]
            need.append((fill.to(torch.int64) + self.pi_stride)[act].sum())
            ctl.append(self.pctl[_native.ZC_TRAJ_PI_ENTRIES])
        npos, ngames, *nent = (int(x) for x in (torch.stack(ctl) + torch.stack(need)).tolist())
        nent = nent[0] if nent else 0
        if npos > self.pool_cap or ngames > self.games_cap or (nent and nent > self.pi_pool_cap):
            grow = lambda need, cap: max(need, cap, 2 * cap if need > cap else 0)  # noqa: E731
            self._grow_pool(grow(ngames, self.games_cap), grow(npos, self.pool_cap),
                            grow(nent, self.pi_pool_cap) if nent else None)

    def start(self, quota: int | None, games_cap: int | None = None):
        """Slot g plays game g (g < quota) or idles; the pool is emptied.  quota None = no
        limit (every finished game's slot starts another).  With a quota the game records are
        sized for it and the positions grow on demand (`ensure_room` before each step), so
        simulate_games never drops a game (round 4 reserved quota x max_len positions up
        front: 2,049 rows per chess game)."""
        q = _UNLIMITED if quota is None else int(quota)
        self.quota = q
        need_g = max(int(games_cap or 0), q if quota is not None else 0)
        if need_g > self.games_cap:
            self._alloc_pool(need_g, self.pool_cap)
        ids = torch.arange(self.n, dtype=torch.int32, device=self.dev)
        self.slot.zero_()
        self.slot[:, 0] = 1
        self.slot[:, 1] = torch.where(ids < min(q, self.n), ids, torch.full_like(ids, -1))
        self.hist[:, 0] = self.init
        self.ctl.zero_()
        self.ctl[_native.ZC_TRAJ_NEXT] = min(q, self.n)
        self.ctl[_native.ZC_TRAJ_QUOTA] = q
        if self.policy_width is not None:
            self.slot_off.zero_()
            self.pctl.zero_()

    def record(self, d_states: int, moves: torch.Tensor, results: torch.Tensor, flags: torch.Tensor | None = None,
               rep: torch.Tensor | None = None, stream: int = 0):
        _native.check(_native.lib().zc_traj_record_async(
            self.n, ctypes.byref(self._buf), ctypes.c_void_p(d_states), ctypes.c_void_p(moves.data_ptr()),
            ctypes.c_void_p(results.data_ptr()), ctypes.c_void_p(flags.data_ptr() if flags is not None else None),
            ctypes.c_void_p(rep.data_ptr() if rep is not None else None), ctypes.c_void_p(stream or None)))
        if self.policy_width is not None:   # the finished games' visit counts follow them into the pool
            _native.check(_native.lib().zc_traj_policy_commit_async(
                self.n, ctypes.byref(self._buf), ctypes.byref(self._pol), ctypes.c_void_p(stream or None)))

    def seed_openings(self, book: torch.Tensor, share: int, roots: torch.Tensor, stream: int = 0):
        """zc_traj_openings_async: every slot whose game has only its first position takes row
        (game number // share) % len(book) of `book` ([N, W] int64 on the device) as its row of
        `roots` and as its history's position 0.  After record() (and its policy commit) of a step
        and after start(); idle slots and games in progress are not touched."""
        _native.check(_native.lib().zc_traj_openings_async(
            self.n, ctypes.byref(self._buf), ctypes.c_void_p(book.data_ptr()), int(book.shape[0]), int(share),
            ctypes.c_void_p(roots.data_ptr()), ctypes.c_void_p(stream or None)))

    def record_policy(self, na: torch.Tensor, root_moves: torch.Tensor | None = None, stream: int = 0):
        """After a step's search, before its play and record(): the root visit counts
        na [n, stride] int32 (d_out_root_na) of the positions searched; chess passes the roots'
        legal-move lists [n, stride] (zc_chess_legal_moves_async), Connect4 nothing (index =
        column)."""
        if self.policy_width is None:
            raise ValueError("this pool records no visit counts (policy_width=None)")
        if tuple(na.shape) != (self.n, self.pi_stride) or na.dtype != torch.int32 or not na.is_contiguous():
            raise ValueError(f"na must be a contiguous int32 [{self.n}, {self.pi_stride}] tensor")
        if root_moves is not None and (tuple(root_moves.shape) != tuple(na.shape) or root_moves.element_size() != 2
                                       or not root_moves.is_contiguous()):
            raise ValueError("root_moves must be a contiguous 16-bit tensor of na's shape")
        _native.check(_native.lib().zc_traj_policy_append_async(
            self.n, ctypes.byref(self._buf), ctypes.byref(self._pol), ctypes.c_void_p(na.data_ptr()),
            ctypes.c_void_p(root_moves.data_ptr() if root_moves is not None else None), self.pi_stride,
            ctypes.c_void_p(stream or None)))

    def record_steps(self, d_states: int, moves: torch.Tensor, results: torch.Tensor, steps: int,
                     reached: torch.Tensor | None = None, stream: int = 0, na: torch.Tensor | None = None,
                     root_moves: torch.Tensor | None = None):
        """record() for `steps` consecutive [steps][n] self-play outputs in one call
        (zc_traj_record_steps_async: four launches whatever `steps` is); only the steps
        k < *reached are read.  Needs the unlimited quota.
        A pool recording the policy needs the launch's staged visit counts na [steps, n, stride]
        int32 (zc_c4_selfplay_visits / zc_chess_selfplay_visits; chess also the staged root moves
        of the same shape, 16-bit): zc_traj_policy_record_steps_async records them first, from
        the slot table the position record then updates."""
        if self.quota != _UNLIMITED:
            raise ValueError("multi-step recording needs the unlimited quota (start(None))")
        if self.policy_width is not None and na is None:
            raise ValueError("the multi-step launches export no per-move visit counts: record the policy with step()")
        if na is not None:
            self._record_policy_steps(results, int(steps), reached, stream, na, root_moves)
        need = ctypes.c_int64(0)
        _native.check(_native.lib().zc_traj_steps_scratch_bytes(self.n, int(steps), ctypes.byref(need)))
        if getattr(self, "_scratch", None) is None or self._scratch.numel() < need.value:
            self._scratch = torch.empty(max(need.value, 16), dtype=torch.uint8, device=self.dev)
        _native.check(_native.lib().zc_traj_record_steps_async(
            self.n, ctypes.byref(self._buf), ctypes.c_void_p(d_states), ctypes.c_void_p(moves.data_ptr()),
            ctypes.c_void_p(results.data_ptr()), int(steps),
            ctypes.c_void_p(reached.data_ptr() if reached is not None else None),
            ctypes.c_void_p(self._scratch.data_ptr()), self._scratch.numel(), ctypes.c_void_p(stream or None)))

    def _record_policy_steps(self, results: torch.Tensor, steps: int, reached: torch.Tensor | None, stream: int,
                             na: torch.Tensor, root_moves: torch.Tensor | None):
        if self.policy_width is None:
            raise ValueError("this pool records no visit counts (policy_width=None)")
        if (na.dim() != 3 or na.shape[0] < steps or tuple(na.shape[1:]) != (self.n, self.pi_stride)
                or na.dtype != torch.int32 or not na.is_contiguous()):
            raise ValueError(f"na must be a contiguous int32 [>= {steps}, {self.n}, {self.pi_stride}] tensor")
        if root_moves is not None and (tuple(root_moves.shape) != tuple(na.shape) or root_moves.element_size() != 2
                                       or not root_moves.is_contiguous()):
            raise ValueError("root_moves must be a contiguous 16-bit tensor of na's shape")
        need = ctypes.c_int64(0)
        _native.check(_native.lib().zc_traj_policy_steps_scratch_bytes(self.n, steps, ctypes.byref(need)))
        if getattr(self, "_pscratch", None) is None or self._pscratch.numel() < need.value:
            self._pscratch = torch.empty(max(need.value, 16), dtype=torch.uint8, device=self.dev)
        _native.check(_native.lib().zc_traj_policy_record_steps_async(
            self.n, ctypes.byref(self._buf), ctypes.byref(self._pol), ctypes.c_void_p(results.data_ptr()),
            ctypes.c_void_p(na.data_ptr()), ctypes.c_void_p(root_moves.data_ptr() if root_moves is not None else None),
            self.pi_stride, steps, ctypes.c_void_p(reached.data_ptr() if reached is not None else None),
            ctypes.c_void_p(self._pscratch.data_ptr()), self._pscratch.numel(), ctypes.c_void_p(stream or None)))

    def finished(self) -> int:
        """Games finished since start() (one device read); raises at once if the pool has
        overflowed (a game was dropped), rather than at take()."""
        fin, ov = (int(x) for x in self.ctl[[_native.ZC_TRAJ_FINISHED, _native.ZC_TRAJ_OVERFLOW]].tolist())
        if ov or (self.policy_width is not None and int(self.pctl[_native.ZC_TRAJ_PI_OVERFLOW])):
            self.take()   # raises with the overflow's cause
        return fin

    def take(self) -> TrajBatch:
        """The pooled games, sorted by game number (start order), as device tensors; the pool
        is emptied (slots keep their games in progress)."""
        ctl = self.ctl.cpu().tolist()
        if ctl[_native.ZC_TRAJ_OVERFLOW]:
            raise RuntimeError("trajectory pool overflow: " + ("pool full (take() more often or raise games_cap) "
                                                               if ctl[_native.ZC_TRAJ_OVERFLOW] & 1 else "")
                               + ("a game longer than max_len " if ctl[_native.ZC_TRAJ_OVERFLOW] & 2 else "")
                               + ("the quota ran out inside a multi-step record" if ctl[_native.ZC_TRAJ_OVERFLOW] & 4
                                  else ""))
        if self.policy_width is not None:
            pov = int(self.pctl[_native.ZC_TRAJ_PI_OVERFLOW])
            if pov:
                raise RuntimeError("policy record overflow: "
                                   + (f"a game's visit counts exceeded pi_slot_cap ({self.pi_slot_cap} entries) "
                                      if pov & 1 else "")
                                   + (f"entry pool full (take() more often or raise pi_pool_cap, {self.pi_pool_cap}) "
                                      if pov & 2 else "")
                                   + (f"a visit count above {_native.ZC_TRAJ_PI_MAX_COUNT} saturated"
                                      if pov & 4 else ""))
        k, n = int(ctl[_native.ZC_TRAJ_GAMES]), int(ctl[_native.ZC_TRAJ_POSITIONS])
        g = self.games[:k]
        order = torch.argsort(g[:, 0])
        g = g[order]
        lens = g[:, 3]
        starts = torch.cumsum(lens, 0) - lens
        idx = torch.repeat_interleave(g[:, 2] - starts, lens, output_size=n) + torch.arange(n, device=self.dev)
        games = torch.stack([g[:, 0], g[:, 1] >> 32, (g[:, 1] & 0xFFFFFFFF) - 1, starts, lens], dim=1)
        out = TrajBatch(self.pool[idx].clone(), self.labels[idx].clone(), self.pool_moves[idx].clone(), games)
        if self.policy_width is not None:   # the entries re-based to the batch's row order
            cnt = self.pool_count[idx].to(torch.int64)
            out.pi_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.dev), torch.cumsum(cnt, 0)])
            total = int(out.pi_off[-1])
            src = torch.repeat_interleave(self.pool_first[idx] - out.pi_off[:-1], cnt, output_size=total)
            out.pi = self.pool_pi[src + torch.arange(total, device=self.dev)]
            self.pctl[_native.ZC_TRAJ_PI_ENTRIES] = 0
        self.ctl[_native.ZC_TRAJ_POSITIONS] = 0
        self.ctl[_native.ZC_TRAJ_GAMES] = 0
        return out


def _room(traj, stream: int | None = None):
    """Before a step under a game quota: grow the trajectory pool so the step cannot overflow
    it (not while a step is being captured into a graph: the unlimited quota is the graphs'
    case, and their pool is pinned).  `stream`: the stream the step runs on (None: torch's
    current one).  The control read and the pool copy run ON that stream, so the read sees the
    previous step's record kernel finished and the copy is ordered before the next one."""
    if traj is None or traj.quota == _UNLIMITED or torch.cuda.is_current_stream_capturing():
        return
    cur = torch.cuda.current_stream(traj.dev)
    if stream is None or stream == cur.cuda_stream:
        traj.ensure_room()
        return
    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=traj.dev)):
        traj.ensure_room()


_NO_FUSED_POLICY = ("the fused multi-step launches export no per-move visit counts: with record_policy=True "
                    "play with step()")


def _warm(search, fn, sims: int):
    """Each part's network once on its own slice of the search's buffers (and at a PolicyNet's
    roots shape: valued._warm_parts), and once at the short last flush's shape
    (NetValue.rows) when the simulations are not a multiple of the batch: kernels loaded and
    buffers allocated before a graph capture."""
    fns = list(fn) if isinstance(fn, (list, tuple)) else [fn]
    valued._warm_parts(search, fns)
    nb, k, n, bs = sims % search.bs, len(fns), search.n, search.bs
    for i, f in enumerate(fns):
        lo, hi = i * n // k, (i + 1) * n // k
        if nb and hasattr(f, "rows"):
            kw = {}
            if getattr(f, "wants_leaves", False):
                kw["leaves"] = search.leaves[lo * bs:hi * bs] if search.leaves is not None else None
            f.rows(search.planes[lo * bs:hi * bs], hi - lo, bs, nb, search.values[lo * bs:hi * bs], **kw)


def _check_eval_merge(eval_merge: bool, net, puct_net):
    """eval_merge's refusals, before the engine: they need no GPU."""
    if not eval_merge:
        return
    if net is None and puct_net is None:
        raise ValueError("eval_merge merges a network's evaluations: it needs net= or puct_net=")
    _check_mfma((net,), (puct_net,), "eval_merge needs", "the network", "merged")


def _check_mfma(value_nets, puct_nets, what="eval_cache / eval_merge need", whose="the network", verb="cached"):
    """The refusal of a value or a PUCT network (None: passed over) that is not in its MFMA form."""
    from . import nets
    for group, kind in ((value_nets, nets.MfmaValueNetwork), (puct_nets, nets.MfmaPolicyValueNetwork)):
        if not all(n is None or isinstance(n, kind) for n in group):
            raise ValueError(f"{what} the MFMA form of {whose} (64 or 128 channels; its tower takes the row count "
                             f"from the device): a torch module cannot be {verb}")


_NO_FUSED_BOOK = ("the fused launches refill from the one opening inside the kernel: a pool with a book of openings "
                  "plays with step()")
_C4_BOTTOM = sum(1 << (7 * c) for c in range(7))
_C4_BOARD = sum(0x3F << (7 * c) for c in range(7))


def _book(openings, game: str) -> torch.Tensor:
    """A pool's openings= argument as [N, W] int64 rows (W = 3: Connect4, 9: chess), where it
    was given; or its refusal.  Connect4 takes a [N, 3] int64 tensor, chess a [N, 72] uint8 tensor
    or a list of FEN strings."""
    if game == "chess" and isinstance(openings, (list, tuple)):
        if not openings or not all(isinstance(f, str) for f in openings):
            raise ValueError("openings: a list of FEN strings must hold at least one, and nothing else")
        rows = np.stack([np.frombuffer(_native.chess_from_fen(f).tobytes(), np.uint8) for f in openings])
        openings = torch.from_numpy(rows.copy())
    width, dtype = (72, torch.uint8) if game == "chess" else (3, torch.int64)
    if not torch.is_tensor(openings) or openings.dim() != 2 or openings.shape[1] != width or openings.dtype != dtype:
        raise ValueError(f"openings must be a [N, {width}] {str(dtype).split('.')[1]} tensor"
                         + (" or a list of FEN strings" if game == "chess" else ""))
    if openings.shape[0] < 1:
        raise ValueError("openings: an empty book")
    if openings.shape[0] > 0x7FFFFFFF:
        raise ValueError("openings: more rows than an int32 counts")
    return openings.contiguous().view(torch.int64) if game == "chess" else openings.contiguous()


def check_c4_book(book: torch.Tensor):
    """Refuses a Connect4 book ([N, 3] int64: stones of the side with turn 0, of the other side,
    turn) that holds a row no game reaches or none can go on from, naming the first: overlapping
    stones, sentinel bits (a column's seventh bit, anything above bit 48), a gap under a stone, a
    turn that is not count(stones[0]) - count(stones[1]) in {0, 1}, four in a row, a full board.
    Torch operations on the book's device; one read back."""
    s0, s1, turn = book[:, 0], book[:, 1], book[:, 2]
    occ = s0 | s1
    bits = torch.arange(49, device=book.device)
    count = lambda x: ((x[:, None] >> bits) & 1).sum(1)   # noqa: E731

    def four(b):
        out = torch.zeros_like(b, dtype=torch.bool)
        for d in (1, 7, 6, 8):
            m = b & (b >> d)
            out |= (m & (m >> (2 * d))) != 0
        return out
    n0, n1 = count(s0 & _C4_BOARD), count(s1 & _C4_BOARD)
    faults = [("overlapping stones", (s0 & s1) != 0),
              ("sentinel bits set", ((occ & ~_C4_BOARD) != 0)),
              ("a gap under a stone", (occ & ~_C4_BOTTOM & ~(occ << 1)) != 0),
              ("turn is not count(stones[0]) - count(stones[1]) in {0, 1}",
               (turn != n0 - n1) | (turn < 0) | (turn > 1)),
              ("a side has four in a row", four(s0) | four(s1)),
              ("a full board", n0 + n1 >= 42)]
    bad = torch.stack([f for _, f in faults]).cpu()
    rows = bad.any(0).nonzero()
    if rows.numel():
        r = int(rows[0])
        raise ValueError(f"openings: row {r}: " + next(name for (name, _), b in zip(faults, bad[:, r]) if b))


def openings_from_games(batch: TrajBatch, ply: int, limit: int | None = None) -> torch.Tensor:
    """A book from finished games: the distinct rows at position index `ply` of every game with
    more than ply + 1 positions (such a position is never a game's last, so never terminal), in
    torch.unique(dim=0)'s order over the row words — the same games give the same book — cut to
    the first `limit`.  Connect4: [N, 3] int64; chess: [N, 72] uint8.  On the batch's device."""
    if ply < 0:
        raise ValueError("ply must be >= 0")
    if limit is not None and limit < 0:
        raise ValueError("limit must be >= 0 or None")
    g = batch.games
    first = g[g[:, 4] > ply + 1, 3] + ply
    rows = batch.rows[first]
    if rows.shape[0]:
        rows = torch.unique(rows, dim=0)
    if limit is not None:
        rows = rows[:limit]
    return rows.contiguous().view(torch.uint8) if rows.shape[1] == 9 else rows


class _SelfPlayPool:
    """What `C4SelfPlay` and `ChessSelfPlay` share: G games of one GPU, the engine and its game
    streams, the three-way search choice of a step (the game's own search kernel, a value
    network, PUCT), the recorder, the captured step graph and the fused multi-move launches.

    A game supplies the attributes below, its state (`roots`, `moves`, ... and `start()`) and
    four launches: `_search` (its own search kernel into moves / na / stats), `_root_moves`
    (the move list that names a root's visit counts), `_play` (play the searched moves; returns
    what `Trajectories.record` is to be given), `_launch` (a fused multi-move launch) and
    `_visits` (register the fused launches' visit-count staging with the engine);
    `_adopt_state` is its share of `adopt()`."""

    MOVE_DTYPE: torch.dtype   # of `moves`, as the game's kernels write them
    NA_WIDTH: int        # moves per root: na's row
    POLICY_WIDTH: int    # Trajectories(policy_width=...)
    POOL_ROWS: int       # pooled positions reserved per game of games_cap
    FUSED_SEARCH: str    # the search of run() / run_pooled(), for their refusal
    record = True        # Connect4 alone can play unrecorded
    _openings_share = 1  # games in a row that start from one opening of the book (an arena: 2)

    def __init__(self, games: int, sims: int, c: float, batch_size: int, seed: int, rank: int, device,
                 temperature: float, record_policy: bool, init_row: torch.Tensor, max_len: int,
                 games_cap: int | None, pi_slot_cap: int | None, pi_pool_cap: int | None,
                 record: bool = True, max_sims: int | None = None, fused_policy: bool = False,
                 eval_cache: int = 0, eval_merge: bool = False, book: torch.Tensor | None = None):
        """The refusals come before the engine: they need no GPU.  book: the game's openings=
        argument as `_book` returns it."""
        if book is not None and not record:   # the rule goes by the recorder's game numbers
            raise ValueError("openings needs the trajectory recorder (record=True): a slot's opening goes by its "
                             "game number")
        if book is not None and fused_policy:
            raise ValueError("openings with fused_policy: " + _NO_FUSED_BOOK)
        if int(eval_cache) < 0:
            raise ValueError(f"eval_cache is a number of entries: 0 (off) or positive (got {eval_cache})")
        self.eval_cache, self.eval_merge, self._caches = int(eval_cache), bool(eval_merge), []
        if record_policy and sims > _native.ZC_TRAJ_PI_MAX_COUNT:   # an entry's count field is 16 bits
            raise ValueError(f"record_policy stores visit counts in 16 bits: sims {sims} > "
                             f"{_native.ZC_TRAJ_PI_MAX_COUNT}")
        if record_policy and not record:   # the entries ride on the trajectories
            raise ValueError("record_policy needs the trajectory recorder (record=True)")
        if fused_policy and not record_policy:   # the switch only lifts the fused launches' refusal
            raise ValueError("fused_policy records the fused launches' visit counts: it needs record_policy=True")
        self.record_policy, self.fused_policy = bool(record_policy), bool(fused_policy)
        self.G, self.sims, self.c, self.bs = games, sims, c, batch_size
        self.dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.eng = _native.NativeEngine(max_games=games, max_sims=max_sims or sims, max_batch=batch_size,
                                        device=self.dev.index or 0)
        self.first_id = rank * games
        self.eng.seed(0, [seed + self.first_id + g for g in range(games)])
        self.moves = torch.zeros(games, dtype=self.MOVE_DTYPE, device=self.dev)
        self.na = torch.zeros((games, self.NA_WIDTH), dtype=torch.int32, device=self.dev)
        self.stats = torch.zeros((games, _native.STATS_FIELDS), dtype=torch.int64, device=self.dev)
        self.results = torch.zeros(games, dtype=torch.int32, device=self.dev)
        self.totals = torch.zeros(2, dtype=torch.int64, device=self.dev)   # expansions, depth sum since reset
        self.traj = None
        if record:
            cap = games_cap or max(8 * games, 1024)
            self.traj = Trajectories(games, init_row, max_len, cap, cap * self.POOL_ROWS, self.dev,
                                     policy_width=self.POLICY_WIDTH if record_policy else None,
                                     pi_slot_cap=pi_slot_cap, pi_pool_cap=pi_pool_cap)
        self.book = book.to(self.dev) if book is not None else None
        self.vs = self.value_fn = self.ps = self.net_fn = None
        self.temperature = float(temperature)
        self._run_k = self._ticket = None

    def _networks(self, net, value_search, value_kw: dict, streams: int,
                  puct_net, puct_search, puct_kw: dict, puct_streams: int):
        """`net=`: the value search and its network; `puct_net=`: the PUCT search and its.  With
        more than one stream, a list of replicas: the games in parts on their own streams
        (valued._split_flushes)."""
        if self.eval_cache and net is None and puct_net is None:
            raise ValueError("eval_cache caches a network's evaluations: it needs net= or puct_net=")
        leaves = bool(self.eval_cache or self.eval_merge)
        if net is not None:
            self.vs = value_search(self.eng, self.G, self.bs, leaves=leaves, **value_kw)
            self.value_fn = self._callables(net, streams, False)
        if puct_net is not None:
            self.ps = puct_search(self.eng, self.G, self.bs, leaves=leaves, **puct_kw)
            self.net_fn = self._callables(puct_net, puct_streams, True)

    def _callables(self, net, k: int, puct: bool):
        """The search's callable over `net`: one, or with k > 1 streams a list over k replicas
        (weights shared, buffers their own).  With eval_cache, evalcache.CachedValue /
        CachedPolicy, every stream's over a table of its own of eval_cache / k entries — parts
        on different streams never share a table — and every table empty: a cache belongs to
        one set of weights.  With eval_merge the caches merge a flush's equal rows
        (EvalCache(merge=True)); without eval_cache they hold no table."""
        reps = [net] if k <= 1 else [net.replica() if hasattr(net, "replica") else net for _ in range(k)]
        if not self.eval_cache and not self.eval_merge:
            fns = [(valued.PolicyNet if puct else valued.NetValue)(r) for r in reps]
            return fns[0] if k <= 1 else fns
        from . import evalcache
        _check_mfma(() if puct else (net,), (net,) if puct else ())
        key_bytes, logit_bytes, entries = self._cache_shape(net, puct, len(reps))
        if [c.logit_bytes for c in self._caches] != [logit_bytes] * len(reps):
            self._caches = [evalcache.EvalCache(entries, key_bytes, logit_bytes, self.dev, merge=self.eval_merge)
                            for _ in reps]
        for c in self._caches:
            c.clear()
        fns = [(evalcache.CachedPolicy if puct else evalcache.CachedValue)(r, c) for r, c in zip(reps, self._caches)]
        return fns[0] if k <= 1 else fns

    def _cache_shape(self, net, puct: bool, tables: int) -> tuple[int, int, int]:
        """(key_bytes: the search's leaf row, logit_bytes: the network's logits row, the entries of
        each of `tables` tables that share eval_cache; 0: no table) of the pool's caches."""
        row, dtype = (self.ps if puct else self.vs).LEAF
        key_bytes = int(np.prod(row)) * torch.empty(0, dtype=dtype).element_size()
        entries = max(self.eval_cache // tables, _native.EVALCACHE_WAYS) if self.eval_cache else 0
        return key_bytes, 2 * net.logits_width if puct else 0, entries

    def eval_cache_stats(self) -> dict:
        """The evaluation caches' counters summed over the streams' tables: {"probed", "hits",
        "inserts", "dropped"} rows since the pool was built, and with eval_merge "merged".
        Synchronises."""
        if not self._caches:
            raise ValueError("this pool was built without eval_cache or eval_merge")
        out = dict.fromkeys(_native.EVALCACHE_MERGED_STATS if self.eval_merge else _native.EVALCACHE_STATS, 0)
        for c in self._caches:
            for k, v in c.stats().items():
                out[k] += v
        return out

    def _stream(self, stream: int | None) -> int:
        return stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream

    def step(self, stream: int | None = None) -> torch.Tensor:
        """One move for every game (on torch's current stream unless given); returns the
        per-game results tensor (ONGOING = 2, IDLE = 3).  Finished games restart from the
        initial position."""
        _room(self.traj, stream)
        self.step_search(stream)
        return self.step_finish(stream)

    def step_search(self, stream: int | None = None) -> torch.Tensor:
        """The search half of a step; returns the results tensor the finish half will fill."""
        s = self._stream(stream)
        if self.ps is not None:
            mv, na, st = self.ps.enqueue(self.roots, self.sims, self.net_fn, temperature=self.temperature)
        elif self.vs is not None:
            mv, na, st = self.vs.enqueue(self.roots, self.sims, self.c, self.value_fn)
        else:
            self._search(s)
            na = self.na
        if na is not self.na:
            self.moves.copy_(mv)
            self.stats.copy_(st)
        if self.record_policy:   # the visit counts of the positions searched, before they are played
            self.traj.record_policy(na, self._root_moves(s), stream=s)
        self.totals += self.stats[:, :2].sum(0)
        return self.results

    def step_finish(self, stream: int | None = None) -> torch.Tensor:
        """Play + evaluate the searched moves, record the positions, refill finished games."""
        s = self._stream(stream)
        rec = self._play(s)
        if rec is not None:
            self.traj.record(*rec, stream=s)
            self._seed_openings(s)
        return self.results

    def _seed_openings(self, s: int):
        """With a book: the slots that hold a game's first position — after start(), or refilled
        by the record just enqueued on `s` — take their game's opening, roots and history.  With
        reuse_tree those slots' kept trees are dropped on the device (zc_*_puct_forget_fresh): an
        opening may sit one or two plies below the last root of the game that ended, and the
        search would re-root into a tree of another game, with its repetition terminals."""
        if self.book is not None:
            self.traj.seed_openings(self.book, self._openings_share, self.roots, stream=s)
            if getattr(self, "reuse_tree", False):
                self.ps.forget_fresh(self.traj.slot, s)

    def capture_step(self):
        """One whole step (search with its network, play, record) as a HIP graph; each
        replay plays the next move of every game."""
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):   # the network's kernels warmed outside the capture
            if self.ps is not None:
                _warm(self.ps, self.net_fn, self.sims)
            elif self.vs is not None:
                _warm(self.vs, self.value_fn, self.sims)
        torch.cuda.current_stream(self.dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.step()
        if self.traj is not None:
            self.traj.pinned = True   # the graph holds the pool's buffers from now on
        return g

    def adopt(self, other):
        """Take over another pool's games in progress: positions (and what else the game keeps
        of them), recorded histories with their visit counts, game numbers; this pool's streams
        and pool stay its own — e.g. a network-mode pool starting from a burned-in pool's mixed
        game ages."""
        self._adopt_state(other)
        if self.traj is None or other.traj is None:
            return
        t, o = self.traj, other.traj
        t.hist.copy_(o.hist)
        t.hmoves.copy_(o.hmoves)
        t.slot.copy_(o.slot)
        t.ctl[_native.ZC_TRAJ_NEXT] = o.ctl[_native.ZC_TRAJ_NEXT]
        if t.policy_width is not None:
            if o.policy_width != t.policy_width or o.pi_slot_cap != t.pi_slot_cap:
                raise ValueError("adopt() with record_policy needs a pool recording the policy with the same "
                                 "pi_slot_cap")
            t.slot_pi.copy_(o.slot_pi)
            t.slot_off.copy_(o.slot_off)

    def _fused(self, moves: int, budget: int | None, stream: int | None, kernel_done, carry: bool = False):
        """run() (budget None) and run_pooled(): the game's `_launch` into the [moves][G] outputs,
        then the recording of every step, in step order.  Needs the unlimited quota
        (start(None)): with a quota the refill depends on other slots' finishes, which step()
        decides once per step.  `kernel_done`: an event recorded after the launch, before the
        recording.  With fused_policy the [moves][G][NA_WIDTH] visit-count staging is allocated
        with the outputs and registered with the engine (`_visits`) before the launch, and the
        recording takes it along."""
        name = "run" if budget is None else "run_pooled"
        if self.book is not None:
            raise ValueError(f"{name}(): " + _NO_FUSED_BOOK)
        if self.record_policy and not self.fused_policy:
            raise ValueError(_NO_FUSED_POLICY)
        if self.traj is not None and self.traj.quota != _UNLIMITED:
            raise ValueError(f"{name}() plays without a game quota; use step() under simulate_games' quota")
        if self.vs is not None or self.ps is not None:
            raise ValueError(f"{name}() fuses the {self.FUSED_SEARCH} search; network modes step()")
        s = self._stream(stream)
        if self._run_k != moves:   # rows shaped like the roots'
            self._run_states = torch.zeros((moves,) + self.roots.shape, dtype=self.roots.dtype, device=self.dev)
            self._run_moves = torch.zeros((moves, self.G), dtype=torch.int16, device=self.dev)
            self._run_results = torch.zeros((moves, self.G), dtype=torch.int32, device=self.dev)
            self._run_na = self._run_root_moves = None
            if self.fused_policy:
                self._run_na = torch.zeros((moves, self.G, self.NA_WIDTH), dtype=torch.int32, device=self.dev)
            self._run_k = moves
        if budget is not None and self._ticket is None:
            self._ticket = torch.zeros(2, dtype=torch.int32, device=self.dev)   # counter, most moves played
        if self.fused_policy:
            self._visits(moves)
        self._launch(moves, budget, carry, s)
        if kernel_done is not None:
            kernel_done.record()
        if self.record:
            self.traj.record_steps(self._run_states.data_ptr(), self._run_moves, self._run_results, moves,
                                   reached=self._ticket[1:] if budget is not None else None, stream=s,
                                   na=self._run_na, root_moves=self._run_root_moves)
        return self._run_results

    def set_network(self, model):
        """Search with `model`'s current weights from the next step() on: the hand-back of the
        learner's loop (learner.full_training_run).  `model` is the trainable module — a
        `nets.ValueNetwork` for a pool built with `net=`, a `nets.PolicyValueNetwork` for one
        built with `puct_net=`; its inference form is built here (learner.inference_form) and
        replaces the pool's value / PUCT callable, every stream's replica included, and every
        evaluation cache (eval_cache) is emptied: a cache belongs to one set of weights.  Kept PUCT
        trees (reuse_tree) hold the old network's priors and values and are dropped.  A step graph
        captured before (`capture_step()`; the caller holds it) has the old network's launches
        baked in: it is not this pool's to drop — capture again.  A pool built without a network
        refuses."""
        from . import learner, nets
        if self.ps is None and self.vs is None:
            raise ValueError("this pool was built without a network (net= / puct_net=): its search takes none")
        puct = self.ps is not None
        if isinstance(model, nets.PolicyValueNetwork) != puct:
            raise TypeError("a puct_net= pool takes a PolicyValueNetwork, a net= pool a ValueNetwork")
        net = learner.inference_form(model, self.dev)
        old = self.net_fn if puct else self.value_fn
        # one replica a stream: weights shared, buffers its own
        new = self._callables(net, len(old) if isinstance(old, (list, tuple)) else 1, puct)
        if puct:
            self.net_fn = new
            if getattr(self, "reuse_tree", False):
                self.ps.forget()
        else:
            self.value_fn = new

    def check(self):
        """Raises what the device collected (chess)."""

    def take(self) -> TrajBatch:
        self.check()
        return self.traj.take()

    def finished_games(self, batch: TrajBatch | None = None):
        """Host view of taken games (tests / inspection): (global slot id, moves, result,
        positions with labels) per game, in start order.  Connect4: columns and [n, 3] rows;
        chess: ((fr, fc, tr, tc), value) moves and [n, 9] int64 rows."""
        return _host_games(batch if batch is not None else self.take(), self.first_id, self._move)

    def close(self):
        self.eng.close()


class C4SelfPlay(_SelfPlayPool):
    """Connect4 self-play pool on one GPU: search (zc_c4_search_async) + play/evaluate
    (zc_c4_play_async) + trajectory recording (zc_traj_record_async), all stream-ordered,
    no host synchronisation per step.  With `net=` the search takes its leaf values from a
    value network (C4ValuedSearch, C2(iii)); with `puct_net=` it is the PUCT search with a
    policy + value network (C4PuctSearch), moves sampled at `temperature`;
    both step() only (the network runs between kernels) and capture_step() into one graph."""

    MAX_LEN = 43   # the opening + at most 42 moves
    MOVE_DTYPE, NA_WIDTH, POLICY_WIDTH, POOL_ROWS, FUSED_SEARCH = torch.int32, 7, 7, MAX_LEN, "rollout"
    _move = staticmethod(int)

    def __init__(self, games: int, sims: int, c: float = 1.4, batch_size: int = 32, seed: int = 0,
                 rank: int = 0, device: int = 0, record: bool = True, games_cap: int | None = None,
                 net=None, puct_net=None, temperature: float = 1.0, puct_seed: int = 1, streams: int = 1,
                 record_policy: bool = False, pi_slot_cap: int | None = None, pi_pool_cap: int | None = None,
                 reuse_tree: bool = False, tree_nodes: int | None = None, fused_policy: bool = False,
                 puct_args: dict | None = None, eval_cache: int = 0, eval_merge: bool = False, openings=None):
        """record_policy: every step()'s root visit counts go with the positions into the
        trajectories (TrajBatch.pi / policy_targets(7)), in every search mode.
        openings: a book of openings, a [N, 3] int64 tensor of positions (`openings_from_games`
        makes one): game g starts from row g % N instead of the empty board
        (zc_traj_openings_async after start() and after every step's record).  The book is checked
        once (`check_c4_book`).  step() and capture_step() only: the fused launches refill inside
        the kernel from the empty board, so run(), run_pooled(), drain(), fused_policy and
        record=False refuse.
        eval_cache (net= / puct_net=, MFMA networks): the entries of a device-resident evaluation
        cache (zeroclone_amd/evalcache.py), split evenly over the streams; a leaf whose position
        was evaluated before takes the stored value and logits and the network runs on the
        others alone.  The moves, visit counts and trajectories are those of the pool without
        it.  0 = off.
        eval_merge (net= / puct_net=, MFMA networks): among the rows of one flush that miss the
        cache, rows holding the same position are evaluated once and the others take a copy
        (EvalCache(merge=True)).  With eval_cache=0 it works alone, without a table and at no
        memory cost.  The pool plays what it plays without it.
        puct_args: C4PuctSearch's c_puct / dirichlet_alpha / dirichlet_eps, where its defaults
        are not wanted.
        fused_policy (needs record_policy): run(), run_pooled() (carry=True too) and drain()
        record them as well — the launch stages every finished move's counts
        (zc_c4_selfplay_visits, [moves][games][7] int32) and zc_traj_policy_record_steps_async
        pools them: the same TrajBatch.pi as the same moves played with step().  Off by default:
        without it the fused launches of a record_policy pool keep refusing.
        reuse_tree (PUCT mode): each search keeps the subtree of the move just played
        (C4PuctSearch(reuse=True)) and adds sims - 1 visits to it; a tree holds up to
        `tree_nodes` nodes (default min(2 * sims, 65534)), and a search whose kept nodes leave
        no room for its own starts afresh.  start() and adopt() drop the kept trees."""
        _check_eval_merge(eval_merge, net, puct_net)
        book = _book(openings, "c4") if openings is not None else None
        if book is not None:
            check_c4_book(book)
        if reuse_tree:
            if puct_net is None:
                raise ValueError("reuse_tree keeps the PUCT search's tree: it needs puct_net")
            # a kept root carries the visits of every earlier search of its game: at most 42 searches
            if record_policy and 42 * sims > _native.ZC_TRAJ_PI_MAX_COUNT:
                raise ValueError(f"record_policy stores visit counts in 16 bits: with reuse_tree a root can hold "
                                 f"42 * sims = {42 * sims} > {_native.ZC_TRAJ_PI_MAX_COUNT} visits")
        super().__init__(games, sims, c, batch_size, seed, rank, device, temperature, record_policy,
                         torch.zeros(24, dtype=torch.uint8), self.MAX_LEN, games_cap, pi_slot_cap, pi_pool_cap,
                         record=record,
                         max_sims=(tree_nodes or min(2 * sims, 65534)) if reuse_tree else None,
                         fused_policy=fused_policy, eval_cache=eval_cache, eval_merge=eval_merge, book=book)
        self.reuse_tree = bool(reuse_tree)
        self.record = record
        self.roots = torch.zeros((games, 3), dtype=torch.int64, device=self.dev)
        self.moves16 = torch.zeros(games, dtype=torch.int16, device=self.dev)
        self.carry_pending = False   # run_pooled(carry=True) left moves in flight (drain() finishes them)
        self._networks(net, valued.C4ValuedSearch, {}, streams,
                       puct_net, valued.C4PuctSearch,
                       dict(seed=puct_seed, reuse=self.reuse_tree, **(puct_args or {})), streams)
        self._seed_openings(self._stream(None))

    def start(self, quota: int | None = None):
        """Every slot back to the opening; with a quota, slots beyond it idle and finished
        slots start new games only while fewer than `quota` have started."""
        if self.carry_pending:   # the games restart: their carried moves are dropped
            # (after every stream's launches: the carry launch may have run on a caller's stream)
            torch.cuda.synchronize(self.dev)
            self.eng.c4_carry_discard(0, self.G, self._stream(None))
            self.carry_pending = False
        self.roots.zero_()
        if self.reuse_tree:
            self.ps.forget()
        if self.traj is not None:
            self.traj.start(quota, games_cap=quota)
            self._seed_openings(self._stream(None))

    def step_search(self, stream: int | None = None) -> torch.Tensor:
        if self.carry_pending:
            raise RuntimeError("moves carried over by run_pooled(carry=True) are in flight: drain() first")
        return super().step_search(stream)

    def _search(self, s: int):
        self.eng.c4_search_async(self.roots.data_ptr(), self.G, self.sims, self.c, self.bs,
                                 self.moves.data_ptr(), self.na.data_ptr(), self.stats.data_ptr(), stream=s)

    def _root_moves(self, s: int):
        return None   # a visit count's index is its column

    def check(self):
        """Raises when a game's last stepwise search failed (a failed search plays no move, so the
        game stays where it is and the next step's search of it fails the same way)."""
        if self.ps is None and self.vs is None:
            return
        bad = self.stats[:, 5].cpu()
        if (bad == _native.ZC_STATUS_INTERNAL).any():
            raise RuntimeError(f"the search of {int((bad == _native.ZC_STATUS_INTERNAL).sum())} game(s) ended with "
                               "ZC_STATUS_INTERNAL: the network returned a non-finite value or logits")

    def _play(self, s: int):
        self.eng.c4_play_async(self.roots.data_ptr(), self.G, self.moves.data_ptr(), self.results.data_ptr(),
                               reset=not self.record, stream=s)
        if not self.record:
            return None
        # on the step's own stream: the copy reads the search's moves and feeds the record
        # kernel, both enqueued on s (torch's current stream would race with a side stream)
        if s == self._stream(None):
            self.moves16.copy_(self.moves)
        else:
            with torch.cuda.stream(torch.cuda.ExternalStream(s, device=self.dev)):
                self.moves16.copy_(self.moves)
        return self.roots.data_ptr(), self.moves16, self.results

    def _adopt_state(self, other: "C4SelfPlay"):
        if self.carry_pending:   # its carried searches belong to the roots being replaced
            raise RuntimeError("moves carried over by run_pooled(carry=True) are in flight: drain() first")
        self.roots.copy_(other.roots)
        if self.reuse_tree:
            self.ps.forget()

    def _visits(self, moves: int):
        self.eng.c4_selfplay_visits(self._run_na.data_ptr(), moves)

    def _launch(self, moves: int, budget: int | None, carry: bool, s: int):
        """zc_c4_selfplay_async / zc_c4_selfplay_pooled_async (carry: zc_c4_selfplay_carry_async);
        either resumes carried moves first."""
        head = (self.roots.data_ptr(), self.G, self.sims, self.c, self.bs, moves)
        outs = (self._run_states.data_ptr(), self._run_moves.data_ptr(), self._run_results.data_ptr(),
                self.stats.data_ptr())
        if budget is None:
            self.eng.c4_selfplay_async(*head, *outs, stream=s)
        else:
            self.eng.c4_selfplay_pooled_async(*head, budget, self._ticket.data_ptr(), *outs, stream=s, carry=carry)
        self.carry_pending = bool(carry)

    def run(self, moves: int, stream: int | None = None, kernel_done=None) -> torch.Tensor:
        """`moves` moves for every game in ONE launch (zc_c4_selfplay_async: each game at its
        own pace, finished games refilled from the opening in the kernel), then the
        trajectory recording of every step, in step order — the same games, pool and labels
        as `moves` calls of step() (with fused_policy their root visit counts too; a
        record_policy pool without it refuses).  Needs the unlimited quota (start(None)).
        Returns the per-step results [moves, G]; self.stats sums the moves' counters."""
        self.results.copy_(self._fused(moves, None, stream, kernel_done)[-1])
        return self._run_results

    def run_pooled(self, budget: int, moves_cap: int, stream: int | None = None, kernel_done=None,
                   carry: bool = False) -> torch.Tensor:
        """`budget` moves shared by all games in ONE launch (zc_c4_selfplay_pooled_async): each
        game takes its next move from a device counter while the budget lasts, at most
        `moves_cap` moves.  A throughput schedule, not the reference's: scripts/train.py:151-170
        is lockstep (one move per unfinished game per call).  Game i's k-th move is the k-th move
        run() would play;
        how many moves each game gets follows the games' pace.  The trajectory recording
        replays the steps in order (slots without a k-th move: ZC_SLOT_SKIP, untouched).
        carry=True (zc_c4_selfplay_carry_async): once the budget is spent the in-flight moves
        stop at their next flush and carry over — the next run()/run_pooled() resumes them
        first; drain() finishes them; step() and the lockstep searches refuse until then.
        With fused_policy every finished move's visit counts are recorded with its position,
        a carried move's by the launch that finishes it.
        Returns the per-step results [moves_cap, G]; self.stats sums the launch's counters."""
        return self._fused(moves_cap, budget, stream, kernel_done, carry)

    def drain(self, stream: int | None = None) -> torch.Tensor:
        """Finish the moves run_pooled(carry=True) left in flight (a pooled launch with no
        budget: each carried move is resumed and finished, nothing new starts), recorded like
        any launch's moves.  Returns that launch's per-step results."""
        return self._fused(1, 0, stream, None)

    def take_positions(self) -> torch.Tensor:
        """Positions of the games finished since the last take, in start order: [n, 3] int64
        device rows (stones X, stones O, turn | Engine.get_dataset label << 32)."""
        return positions_of(self.take())


def positions_of(b: TrajBatch) -> torch.Tensor:
    """A Connect4 TrajBatch as the exchange's rows: [n, 3] int64 (stones X, stones O,
    turn | Engine.get_dataset label << 32), on the batch's device."""
    rows = b.rows.clone()
    rows[:, 2] = (rows[:, 2] & 1) | (b.labels.to(torch.int64) << 32)
    return rows


def _host_games(b: TrajBatch, first_id: int, move_fn):
    rows, labels, moves = b.rows.cpu().numpy(), b.labels.cpu().numpy(), b.moves.cpu().numpy()
    out = []
    for gno, slot, res, off, n in b.games.cpu().numpy().tolist():
        pos = rows[off:off + n].copy()
        if pos.shape[1] == 3:
            pos[:, 2] = (pos[:, 2] & 1) | (labels[off:off + n].astype(np.int64) << 32)
        out.append((first_id + slot, [move_fn(m) for m in moves[off:off + n - 1]], res, pos))
    return out


class ChessSelfPlay(_SelfPlayPool):
    """Device-resident chess self-play: the chess form of `C4SelfPlay`.  G games live on one
    GPU as zc_chess_state rows; one `step()` searches every game — Value('crude_chess_score')
    in the search kernel, a value network between the stepwise select and backup kernels
    (`net=`), or the PUCT search with a policy + value network (`puct_net=`)
    — then ONE kernel plays the chosen moves, tests the new positions (check_win, stalemate,
    the fifty-move rule) and both sides' move histories (the repetition half of check_draw,
    chess_backend.cpp:416-441; histories in HBM) and refills finished games
    (zc_chess_play_step_async), and the recorder pools the finished games
    (zc_traj_record_async: Engine._evaluate's results, engine.py:148-153).  With the crude
    score, `run(K)` / `run_pooled(budget, cap)` play K moves per game (or a shared budget) in
    ONE launch (zc_chess_selfplay*_async) — the same games as K steps.  Nothing is read back
    per step; errors (a game longer than the history capacity, a search out of tree
    capacity, no move at a live root) are collected on the device and raised by `check()` /
    `take()`.  `capture_step()` records a whole step (search, network, play, record) in one
    HIP graph."""

    MOVE_DTYPE, NA_WIDTH, POLICY_WIDTH, POOL_ROWS = torch.int16, _native.CHESS_MAX_MOVES, 4096, 160
    FUSED_SEARCH = "crude-score"
    _move = staticmethod(lambda m: _native.unpack_chess_move(int(m) & 0xFFFF))

    def __init__(self, games: int, sims: int, c: float = 1.4, batch_size: int = 32, seed: int = 0,
                 rank: int = 0, device: int = 0, policy: int = _native.ZC_POLICY_IMMEDIATE_VALUE,
                 freedom: float = 3.0, net=None, init_fen: str | None = None, games_cap: int | None = None,
                 hist_cap: int = 1024, puct_net=None, temperature: float = 1.0, puct_seed: int = 1,
                 puct_streams: int = 1, streams: int = 1, record_policy: bool = False,
                 pi_slot_cap: int | None = None, pi_pool_cap: int | None = None,
                 reuse_tree: bool = False, tree_nodes: int | None = None, fused_policy: bool = False,
                 puct_args: dict | None = None, eval_cache: int = 0, eval_merge: bool = False, openings=None):
        """record_policy: every step()'s root visit counts go with the positions into the
        trajectories (TrajBatch.pi / policy_targets(4096)), in every search mode.
        openings: as C4SelfPlay's; a [N, 72] uint8 tensor of zc_chess_state rows or a list of FEN
        strings.  An opening starts with empty repetition histories, as init_fen= does, and its
        fifty-move counter and castling rights are the row's own.  A row that
        zc_chess_terminal_async flags (no legal move, the fifty-move rule reached) is refused.
        eval_cache: as C4SelfPlay's (with the convolutional head an entry holds 8 KB of logits).
        eval_merge: as C4SelfPlay's.
        puct_args: ChessPuctSearch's c_puct / dirichlet_alpha / dirichlet_eps, where its defaults
        are not wanted.
        fused_policy (needs record_policy): run() and run_pooled() record them as well — the
        launch stages every move's counts and root moves (zc_chess_selfplay_visits,
        [moves][games][256] int32 + int16: about 63 MB at 60 steps x 1024 games) and
        zc_traj_policy_record_steps_async pools them: the same TrajBatch.pi as the same moves
        played with step().  Off by default: without it the fused launches of a record_policy
        pool keep refusing.
        reuse_tree (PUCT mode): each search keeps the subtree of the move just played
        (ChessPuctSearch(reuse=True)) and adds sims - 1 visits to it; a tree holds up to
        `tree_nodes` nodes (default min(2 * sims, 65534)) and 64 child slots per node, and a
        search whose kept nodes or slots leave no room for its own starts afresh.  start() and
        adopt() drop the kept trees.  With record_policy a kept root's visit counts can exceed
        sims (a chess game has no fixed length, so no bound is refused here): a count beyond 16
        bits is recorded saturated and sets the recorder's ZC_TRAJ_PI_OVERFLOW bit 2."""
        _check_eval_merge(eval_merge, net, puct_net)
        if reuse_tree and puct_net is None:
            raise ValueError("reuse_tree keeps the PUCT search's tree: it needs puct_net")
        book = _book(openings, "chess") if openings is not None else None
        init = _native.chess_from_fen(init_fen) if init_fen else _native.chess_init()
        init = torch.from_numpy(np.frombuffer(init.tobytes(), np.uint8).reshape(1, 72).copy())
        max_len = 2 * hist_cap + 1
        if record_policy and pi_slot_cap is None:   # a position has at most min(sims, 256) visited moves
            # (a kept root brings the visits of earlier searches: up to every move)
            pi_slot_cap = (max_len - 1) * (_native.CHESS_MAX_MOVES if reuse_tree else min(sims, _native.CHESS_MAX_MOVES))
        super().__init__(games, sims, c, batch_size, seed, rank, device, temperature, record_policy,
                         init, max_len, games_cap, pi_slot_cap, pi_pool_cap,
                         max_sims=(tree_nodes or min(2 * sims, 65534)) if reuse_tree else None,
                         fused_policy=fused_policy, eval_cache=eval_cache, eval_merge=eval_merge, book=book)
        self.reuse_tree = bool(reuse_tree)
        self.eng.chess_reserve()
        self.policy, self.freedom = int(policy), float(freedom)
        self.init_row = init.to(self.dev)
        self.roots = self.init_row.repeat(games, 1).contiguous()
        self.post = torch.zeros_like(self.roots)
        # a network with the convolutional head takes the planes in its input layout straight
        # from the select kernel (no conversion launch per flush)
        nhwc = bool(getattr(puct_net, "conv_head", False)) and os.environ.get("ZC_PUCT_NHWC", "1") != "0"   # 0: A/B
        self._networks(net, valued.ChessValuedSearch, dict(policy=self.policy, freedom=self.freedom), streams,
                       puct_net, valued.ChessPuctSearch,
                       dict(seed=puct_seed, planes_nhwc=nhwc, reuse=self.reuse_tree, **(puct_args or {})), puct_streams)
        self.hist_cap = hist_cap  # moves per side
        self.hist = torch.zeros((games, 2, self.hist_cap), dtype=torch.int16, device=self.dev)
        self.hlen = torch.zeros((games, 2), dtype=torch.int32, device=self.dev)
        self.err = torch.zeros(3, dtype=torch.int32, device=self.dev)
        b = _native.ChessPlayBuffers()
        b.d_roots, b.d_init, b.d_hist = self.roots.data_ptr(), self.init_row.data_ptr(), self.hist.data_ptr()
        b.d_hist_len, b.hist_cap, b.d_err = self.hlen.data_ptr(), self.hist_cap, self.err.data_ptr()
        self._pb = b
        if record_policy:
            self.root_moves = torch.zeros((games, _native.CHESS_MAX_MOVES), dtype=torch.int16, device=self.dev)
            self.root_counts = torch.zeros(games, dtype=torch.int32, device=self.dev)
        if self.book is not None:
            self._check_book()
            self._seed_openings(self._stream(None))

    def _check_book(self):
        """Once per book: zc_chess_terminal_async over its rows, read back."""
        flags = torch.zeros(self.book.shape[0], dtype=torch.int32, device=self.dev)
        self.eng.chess_terminal_async(self.book.shape[0], self.book.data_ptr(), flags.data_ptr(), self._stream(None))
        bad = flags.cpu().nonzero()
        if bad.numel():
            r = int(bad[0])
            f = int(flags[r])
            why = [name for bit, name in ((_native.ZC_CHESS_WIN, "the side to move is mated"),
                                          (_native.ZC_CHESS_STALEMATE, "no legal move"),
                                          (_native.ZC_CHESS_FIFTY, "the fifty-move rule is reached"),
                                          (_native.ZC_CHESS_OVERFLOW, "more legal moves than a move list holds"))
                   if f & bit]
            self.close()
            raise ValueError(f"openings: row {r} is not a position a game starts from: " + ", ".join(why))

    def start(self, quota: int | None = None):
        self.roots.copy_(self.init_row.expand_as(self.roots))
        self.hlen.zero_()
        if self.reuse_tree:
            self.ps.forget()
        self.traj.start(quota, games_cap=quota)
        self._seed_openings(self._stream(None))

    def _search(self, s: int):
        self.eng.chess_search_async(0, self.G, self.roots.data_ptr(), self.sims, self.c, self.bs, self.policy,
                                    self.freedom, self.moves.data_ptr(), self.na.data_ptr(),
                                    self.stats.data_ptr(), s)

    def _root_moves(self, s: int):
        """The roots' legal-move lists name the visit counts' moves (before the play)."""
        self.eng.chess_legal_moves_async(self.G, self.roots.data_ptr(), self.root_moves.data_ptr(),
                                         self.root_counts.data_ptr(), s)
        return self.root_moves

    def _play(self, s: int):
        _native.check(_native.lib().zc_chess_play_step_async(
            self.G, ctypes.byref(self._pb), ctypes.c_void_p(self.moves.data_ptr()),
            ctypes.c_void_p(self.stats.data_ptr()), ctypes.c_void_p(self.post.data_ptr()),
            ctypes.c_void_p(self.results.data_ptr()), ctypes.c_void_p(s)))
        return self.post.data_ptr(), self.moves, self.results

    def _adopt_state(self, other: "ChessSelfPlay"):
        """Beside the positions, both sides' move histories (the repetition draw)."""
        if other.hist_cap != self.hist_cap:
            raise ValueError("adopt() needs the same hist_cap")
        self.roots.copy_(other.roots)
        self.hist.copy_(other.hist)
        self.hlen.copy_(other.hlen)
        if self.reuse_tree:
            self.ps.forget()

    def _visits(self, moves: int):
        """Chess names a root's visit counts by the root's moves, staged beside them."""
        if self._run_root_moves is None:
            self._run_root_moves = torch.zeros(tuple(self._run_na.shape), dtype=torch.int16, device=self.dev)
        self.eng.chess_selfplay_visits(self._run_na.data_ptr(), self._run_root_moves.data_ptr(), moves)

    def _launch(self, moves: int, budget: int | None, carry: bool, s: int):
        """zc_chess_selfplay_async / zc_chess_selfplay_pooled_async."""
        head = [self.eng.handle, 0, self.G, ctypes.byref(self._pb), self.sims, self.c, self.bs, self.policy,
                self.freedom, moves]
        outs = [ctypes.c_void_p(self._run_states.data_ptr()), ctypes.c_void_p(self._run_moves.data_ptr()),
                ctypes.c_void_p(self._run_results.data_ptr()), ctypes.c_void_p(self.stats.data_ptr()),
                ctypes.c_void_p(s)]
        if budget is None:
            _native.check(_native.lib().zc_chess_selfplay_async(*head, *outs))
        else:
            _native.check(_native.lib().zc_chess_selfplay_pooled_async(
                *head, int(budget), ctypes.c_void_p(self._ticket.data_ptr()), *outs))

    def run(self, moves: int, stream: int | None = None, kernel_done=None) -> torch.Tensor:
        """Crude score: `moves` moves for every game in ONE launch (zc_chess_selfplay_async),
        then the multi-step recording — the same games, pool and labels as `moves` calls of
        step() (with fused_policy their root visit counts too; a record_policy pool without it
        refuses).  Returns the per-step results [moves, G]; self.stats sums the moves."""
        return self._fused(moves, None, stream, kernel_done)

    def run_pooled(self, budget: int, moves_cap: int, stream: int | None = None, kernel_done=None) -> torch.Tensor:
        """Crude score: `budget` moves shared by the games in ONE launch (at most moves_cap
        each; a throughput schedule, the reference's train.py is lockstep).  Game i's k-th
        move is the k-th move run() would play."""
        return self._fused(moves_cap, budget, stream, kernel_done)

    def check(self):
        e = self.err.cpu().tolist()
        if e[0]:
            raise RuntimeError(f"a game exceeded {self.hist_cap} moves per side")
        if e[1] & 2:
            raise RuntimeError(f"a played position's legal-move list overflowed {_native.CHESS_MAX_MOVES} moves "
                               "(the game was not judged)")
        if e[1]:
            raise RuntimeError("chess search exceeded the tree's child-slot pool or depth limit")
        if e[2]:   # a search handed over no move: its status was not 0
            raise RuntimeError("a search returned no move for a live game: no legal move at a non-terminal root, or "
                               "(PUCT) the network returned a non-finite value or logits (ZC_STATUS_INTERNAL)")


def simulate_games(pool, total_games: int, max_steps: int | None = None, check_every: int = 4) -> list[int]:
    """scripts/train.py:simulate_games (:151-170) on a device pool (C4SelfPlay or
    ChessSelfPlay): games 0..min(total, G)-1 start in slots 0.., a finished game's slot starts
    the next game while fewer than `total_games` have started, and every started game is
    played to its end.  Returns the results by game number (start order), as the
    reference's `final` list; the games' trajectories stay in the pool (`pool.take()`)."""
    if total_games < 0:
        raise ValueError("total_games must be >= 0")
    pool.start(total_games)
    steps = 0
    while total_games and (steps % check_every or pool.traj.finished() < total_games):
        if max_steps is not None and steps >= max_steps:
            raise RuntimeError(f"{pool.traj.finished()} of {total_games} games finished in {max_steps} steps")
        pool.step()   # with a quota, step() grows the trajectory pool first (ensure_room)
        steps += 1
    pool.last_batch = pool.take()
    res = pool.last_batch.results()
    assert len(res) == total_games, (len(res), total_games)
    return res


def schedule_hyperparams(cycle: int, *, games_cap: int = 2000, sims_cap: int = 800, init_lr: float = 3e-4,
                         lr_decay: float = 0.95, lr_floor: float = 1e-5) -> dict:
    """scripts/train.py:schedule_hyperparams (:173-188): the self-play games, simulations per
    move and exploration constant of training cycle `cycle`, and its learning rate."""
    games = min(games_cap, 500 * (cycle + 1))
    sims = int(min(100 * (1.2 ** cycle), sims_cap))
    c_val = max(1.25, 2.5 * (0.97 ** cycle))
    lr = max(init_lr * (lr_decay ** cycle), lr_floor)
    return {"games": games, "simulations": sims, "c_puct": c_val, "lr": lr}


def gather_positions(local: torch.Tensor, group=None) -> torch.Tensor:
    """All-gather variable-length [n_r, ...] position rows from every rank (rank order; e.g.
    [n, 3] int64 Connect4 rows with labels, or chess rows): an all_gather of the counts,
    then of payloads padded to the largest count."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    n = torch.tensor([local.shape[0]], dtype=torch.int64, device=local.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n, group=group)
    counts = [int(c.item()) for c in counts]
    m = max(counts) if counts else 0
    pad = torch.zeros((m,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    bufs = [torch.zeros_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad, group=group)
    return torch.cat([b[:c] for b, c in zip(bufs, counts)], dim=0)


class ReplayBuffer:
    """scripts/train.py:_update_replay (:27-50): the training set of a cycle = a uniform
    sample (without replacement) of 30 % of everything seen before, then all new data.

    Works on numpy arrays or device tensors (the pooled positions stay on the GPU: the old
    data is concatenated and indexed on the device).  The sample indices come from numpy's
    GLOBAL generator, `np.random.choice(len(old), k, replace=False)`, exactly the
    reference's call — so after the same `np.random.seed` the same rows are drawn; pass
    `seed` for a private generator instead."""

    def __init__(self, frac_old: float = 0.30, seed: int | None = None):
        self.frac_old = frac_old
        self.states, self.values = [], []
        self.rng = np.random.default_rng(seed) if seed is not None else None

    @staticmethod
    def _cat(xs):
        return torch.cat(xs, dim=0) if torch.is_tensor(xs[0]) else np.concatenate(xs, axis=0)

    def update(self, states_new, values_new):
        if not self.states:
            self.states.append(states_new)
            self.values.append(values_new)
            return states_new, values_new
        old_s, old_v = self._cat(self.states), self._cat(self.values)
        k = int(self.frac_old * len(old_s))
        if k > 0:
            idx = (self.rng.choice(len(old_s), k, replace=False) if self.rng is not None
                   else np.random.choice(len(old_s), k, replace=False))
            if torch.is_tensor(old_s):
                idx = torch.from_numpy(idx).to(old_s.device)
            ss, sv = old_s[idx], old_v[idx]
        else:
            ss, sv = old_s[:0], old_v[:0]
        self.states.append(states_new)
        self.values.append(values_new)
        return self._cat([ss, states_new]), self._cat([sv, values_new])
