"""ctypes binding of libzeroclone_amd.so (the C-ABI in include/zeroclone.h).

There is no CPU fallback: if the library or a GPU is missing, constructing an engine raises.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import threading
import types

import numpy as np

from .build import LIB

P = ctypes.POINTER

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zeroclone.h")

# The header's whole type vocabulary: these scalars, `const char *` (c_char_p), and pointers to
# anything (c_void_p: it takes byref(), arrays, typed pointers, ints and None alike).
_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "uint32_t": ctypes.c_uint32, "double": ctypes.c_double, "float": ctypes.c_float, "int": ctypes.c_int}


@functools.lru_cache(maxsize=None)
def _ctype(text: str):
    """The ctypes type of one return type or parameter, its name, if any, included."""
    words = re.findall(r"\w+|\*", text)
    if not words or not re.fullmatch(r"[\w\s*]+", text):
        raise ValueError(f"cannot read {text.strip()!r}")
    if "*" in words:
        return ctypes.c_char_p if words[:3] == ["const", "char", "*"] and words.count("*") == 1 else ctypes.c_void_p
    if words[0] not in _SCALARS or len(words) > 2:
        raise ValueError(f"unknown type {text.strip()!r}")
    return _SCALARS[words[0]]


def parse_header(text: str):
    """(signatures, constants) of a header's text: a (name, restype, argtypes) for every
    `<ret> zc_name(<params>);` and the value of every `#define ZC_NAME <int>`.  A declaration
    that is not understood is an error naming it, never a guess: a wrong argtype corrupts a call
    without a sign."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(ZC_\w+)[ \t]+(-?\d+)[ \t]*$", text,
                                                      re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', " ", text, flags=re.M)
    signatures = []
    for stmt in text.split(";"):
        if not re.search(r"\bzc_\w+\s*\(", stmt):
            continue
        decl = " ".join(stmt.split())
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(zc_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            raise ValueError(f"{HEADER}: cannot split the declaration {decl!r}")
        try:
            restype, *argtypes = [_ctype(t) for t in ([m[1]] if m[3].strip() == "void" else [m[1], *m[3].split(",")])]
        except ValueError as e:
            raise ValueError(f"{HEADER}: {e} in the declaration {decl!r}") from None
        signatures.append((m[2], restype, argtypes))
    return signatures, constants


# Every function and every integer constant include/zeroclone.h declares, read from it once per
# process: SIGNATURES as (name, restype, argtypes), the constants under their header names.
with open(HEADER) as _f:
    SIGNATURES, CONSTANTS = parse_header(_f.read())
globals().update(CONSTANTS)
ROLLOUT_EXACT, ROLLOUT_PHILOX = CONSTANTS["ZC_ROLLOUT_EXACT"], CONSTANTS["ZC_ROLLOUT_PHILOX"]


class C4State(ctypes.Structure):
    _fields_ = [("stones", ctypes.c_uint64 * 2), ("turn", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class GameStats(ctypes.Structure):
    _fields_ = [("expansions", ctypes.c_int64), ("depth_sum", ctypes.c_int64), ("leaves", ctypes.c_int64),
                ("rollout_plies", ctypes.c_int64), ("rng_words", ctypes.c_int64), ("status", ctypes.c_int64),
                ("rollout_blocks", ctypes.c_int64), ("reserved", ctypes.c_int64)]


class EngineConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("max_games", ctypes.c_int32), ("max_sims", ctypes.c_int32),
                ("max_batch", ctypes.c_int32)]


class ChessPlayBuffers(ctypes.Structure):
    """zc_chess_play_buffers (include/zeroclone.h): a chess self-play pool's device buffers."""
    _fields_ = [("d_roots", ctypes.c_void_p), ("d_init", ctypes.c_void_p), ("d_hist", ctypes.c_void_p),
                ("d_hist_len", ctypes.c_void_p), ("hist_cap", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("d_err", ctypes.c_void_p)]


class TrajBuffers(ctypes.Structure):
    """zc_traj_buffers (include/zeroclone.h): device pointers of a self-play trajectory pool."""
    _fields_ = [("row_bytes", ctypes.c_int32), ("max_len", ctypes.c_int32), ("pool_cap", ctypes.c_int64),
                ("games_cap", ctypes.c_int32), ("reserved", ctypes.c_int32), ("d_hist", ctypes.c_void_p),
                ("d_hmoves", ctypes.c_void_p), ("d_slot", ctypes.c_void_p), ("d_pool", ctypes.c_void_p),
                ("d_labels", ctypes.c_void_p), ("d_pool_moves", ctypes.c_void_p), ("d_games", ctypes.c_void_p),
                ("d_ctl", ctypes.c_void_p), ("d_init", ctypes.c_void_p)]


class TrajPolicyBuffers(ctypes.Structure):
    """zc_traj_policy_buffers (include/zeroclone.h): the sparse root-visit-count record kept beside a
    trajectory pool."""
    _fields_ = [("slot_cap", ctypes.c_int32), ("reserved", ctypes.c_int32), ("pi_pool_cap", ctypes.c_int64),
                ("d_slot_pi", ctypes.c_void_p), ("d_slot_off", ctypes.c_void_p), ("d_slot_base", ctypes.c_void_p),
                ("d_pool_pi", ctypes.c_void_p), ("d_pool_first", ctypes.c_void_p), ("d_pool_count", ctypes.c_void_p),
                ("d_pctl", ctypes.c_void_p)]


class TrainSet(ctypes.Structure):
    """zc_train_set (include/zeroclone.h): a compact training set's device pointers."""
    _fields_ = [("game", ctypes.c_int32), ("row_bytes", ctypes.c_int32), ("n_rows", ctypes.c_int64),
                ("d_rows", ctypes.c_void_p), ("d_labels", ctypes.c_void_p), ("d_pi_off", ctypes.c_void_p),
                ("d_pi", ctypes.c_void_p)]


ZC_TRAJ_PI_MAX_COUNT = 65535   # a policy entry's count field: 16 bits (not in the header)

C4_STATE_DTYPE = np.dtype([("stones", "<u8", (2,)), ("turn", "<i4"), ("reserved", "<i4")])
# zc_c4_hp_node: the host-policy walk's end (include/zeroclone.h)
C4_HP_NODE_DTYPE = np.dtype([("state", C4_STATE_DTYPE), ("node", "<i4"), ("n_untried", "<i4"), ("depth", "<i4"),
                             ("untried", "<i4", (7,))])
STATS_DTYPE = np.dtype([("expansions", "<i8"), ("depth_sum", "<i8"), ("leaves", "<i8"),
                        ("rollout_plies", "<i8"), ("rng_words", "<i8"), ("status", "<i8"),
                        ("rollout_blocks", "<i8"), ("reserved", "<i8")])
CHESS_STATE_DTYPE = np.dtype([("board", "u1", (64,)), ("turn", "u1"), ("fifty", "u1"), ("castle", "u1"),
                              ("reserved", "u1", (5,))])
CHESS_MAX_MOVES = CONSTANTS["ZC_CHESS_MAX_MOVES"]
CHESS_ROLL_CAP = CONSTANTS["ZC_CHESS_ROLL_CAP"]   # moves per side a chess rollout's history holds
# zc_chess_hp_node: the chess host-policy walk's end (include/zeroclone.h)
CHESS_HP_NODE_DTYPE = np.dtype([("state", CHESS_STATE_DTYPE), ("node", "<i4"), ("n_untried", "<i4"), ("depth", "<i4"),
                                ("reserved", "<i4"), ("untried", "<u2", (CHESS_MAX_MOVES,))])
# ChessNode (zc_internal.h): the device tree's node record, as zc_debug_chess_tree copies it
CHESS_NODE_DTYPE = np.dtype([("st", "u1", (72,)), ("base", "<u4"), ("nmoves", "<u2"), ("nu", "<u2"),
                             ("parent", "<u2"), ("pact", "<u2"), ("depth", "<u2"), ("material", "<i2"),
                             ("check", "u1"), ("evaluated", "u1"), ("pad", "u1", (6,))])
assert CHESS_NODE_DTYPE.itemsize == 96
# C4PNode (zc_internal.h): the Connect4 PUCT tree's node record
C4_PNODE_DTYPE = np.dtype([("s0", "<u8"), ("s1", "<u8"), ("order", "<u4"), ("turn", "u1"), ("nmoves", "u1"),
                           ("evaluated", "u1"), ("won", "u1"), ("parent", "<u2"), ("pact", "u1"), ("depth", "u1"),
                           ("pad0", "<u4"), ("child", "<u2", (8,)), ("na", "<i4", (8,)), ("pr", "<f4", (8,)),
                           ("w", "<f8", (8,)), ("pad1", "u1", (16,))])
assert C4_PNODE_DTYPE.itemsize == 192
assert CHESS_STATE_DTYPE.itemsize == 72
assert C4_STATE_DTYPE.itemsize == ctypes.sizeof(C4State) == 24
assert STATS_DTYPE.itemsize == ctypes.sizeof(GameStats) == 64
STATS_FIELDS = 8

_lib = None
_lock = threading.Lock()
# The entry points of each game's searches by their name after the prefix (_C4.ext_begin is
# zc_c4_ext_begin), filled in by lib(): the stepwise wrappers below are written once for both
# games and take one of these, so a call looks nothing up by name.
_C4, _CHESS = types.SimpleNamespace(), types.SimpleNamespace()


class ZeroCloneError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[zc {code}] {msg}")
        self.code = code


def lib(build_if_missing: bool = True):
    """Load libzeroclone_amd.so (building it with hipcc if absent and allowed)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB):
                if not build_if_missing:
                    raise ImportError(f"{LIB} not built (run python -m zeroclone_amd.build)")
                from .build import build
                build()
            L = ctypes.CDLL(LIB)
            for name, res, args in SIGNATURES:
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
                for game, fns in (("zc_c4_", _C4), ("zc_chess_", _CHESS)):
                    if name.startswith(game):
                        setattr(fns, name[len(game):], fn)
            _lib = L
    return _lib


def check(rc: int):
    if rc < 0:
        msg = lib().zc_last_error().decode(errors="replace")
        if rc == ZC_EINVAL:
            raise ValueError(msg)
        raise ZeroCloneError(rc, msg)
    return rc


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


def device_count() -> int:
    n = ctypes.c_int32(0)
    check(lib().zc_device_count(ctypes.byref(n)))
    return n.value


def c4_from_rows(rows42: str, turn: int) -> np.void:
    s = C4State()
    check(lib().zc_c4_from_rows(rows42.encode(), int(turn), ctypes.byref(s)))
    out = np.zeros((), C4_STATE_DTYPE)
    out["stones"] = (s.stones[0], s.stones[1])
    out["turn"] = s.turn
    return out


def c4_legal_order(mask: int) -> list[int]:
    cols = (ctypes.c_int32 * 7)()
    n = check(lib().zc_c4_legal_order(int(mask), cols))
    return list(cols[:n])


def chess_from_fen(fen: str) -> np.ndarray:
    out = np.zeros(1, CHESS_STATE_DTYPE)
    check(lib().zc_chess_from_fen(fen.encode(), _ptr(out)))
    return out[0]


def chess_init() -> np.ndarray:
    out = np.zeros(1, CHESS_STATE_DTYPE)
    check(lib().zc_chess_init(_ptr(out)))
    return out[0]


def unpack_chess_move(m: int):
    """uint16 move -> ((fr, fc, tr, tc), capture value)."""
    m = int(m)
    f, t = m & 63, (m >> 6) & 63
    return (f >> 3, f & 7, t >> 3, t & 7), float((m >> 12) & 15)


def pack_chess_move(fr: int, fc: int, tr: int, tc: int, value: float) -> int:
    return (fr * 8 + fc) | ((tr * 8 + tc) << 6) | (int(value) << 12)


ARENA_ROUTE_THREADS = CONSTANTS["ZC_ARENA_ROUTE_THREADS"]   # the route kernel's workgroup, and its chunk of keys


def _arena_rc(name: str, rc: int):
    """The arena entry points record no message (include/zeroclone.h): the wrappers below check
    what the library checks, so a code from it is a launch error."""
    if rc == ZC_EINVAL:
        raise ValueError(f"{name}: bad argument")
    if rc < 0:
        raise ZeroCloneError(rc, f"{name}: the launch failed")


def arena_route(n: int, d_key: int, d_perm: int, d_count: int, stream: int = 0):
    """zc_arena_route_async on device pointers: d_perm[n] int32 = the stable partition of 0..n-1 by
    d_key[i] & 1, d_count[2] int32 = the group sizes.  Only enqueues."""
    if n < 0:
        raise ValueError(f"n must be >= 0 (got {n})")
    if not d_count or (n and not (d_key and d_perm)):
        raise ValueError("zc_arena_route_async: null device pointer")
    _arena_rc("zc_arena_route_async", lib().zc_arena_route_async(
        int(n), ctypes.c_void_p(d_key), ctypes.c_void_p(d_perm), ctypes.c_void_p(d_count), ctypes.c_void_p(stream or None)))


def _arena_copy(fn_name: str, n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, stream):
    if n < 0 or not 1 <= rows <= game_rows:
        raise ValueError(f"{fn_name}: need n >= 0 and 1 <= rows <= game_rows (got n {n}, rows {rows}, "
                         f"game_rows {game_rows})")
    if row_bytes < 2 or row_bytes % 2 or row_bytes >= 1 << 31:
        raise ValueError(f"{fn_name}: row_bytes must be a positive multiple of 2 below 2^31 (got {row_bytes})")
    if n * game_rows >= 1 << 31:
        raise ValueError(f"{fn_name}: n * game_rows must be < 2^31")
    if n and not (d_perm and d_src and d_dst):
        raise ValueError(f"{fn_name}: null device pointer")
    if (d_src | d_dst) & 1:
        raise ValueError(f"{fn_name}: source and destination must be 2-byte aligned")
    _arena_rc(fn_name, getattr(lib(), fn_name)(
        int(n), int(rows), int(game_rows), int(row_bytes), ctypes.c_void_p(d_perm), ctypes.c_void_p(d_src),
        ctypes.c_void_p(d_dst), ctypes.c_void_p(stream or None)))


def arena_gather(n: int, rows: int, game_rows: int, row_bytes: int, d_perm: int, d_src: int, d_dst: int,
                 stream: int = 0):
    """zc_arena_gather_async: row d_perm[i] * game_rows + j of d_src -> row i * rows + j of d_dst
    (i < n, j < rows).  Only enqueues."""
    _arena_copy("zc_arena_gather_async", n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, stream)


def arena_scatter(n: int, rows: int, game_rows: int, row_bytes: int, d_perm: int, d_src: int, d_dst: int,
                  stream: int = 0):
    """zc_arena_scatter_async: the inverse of arena_gather (row i * rows + j of d_src -> row
    d_perm[i] * game_rows + j of d_dst; a game's rows j >= rows are left untouched)."""
    _arena_copy("zc_arena_scatter_async", n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, stream)


EVALCACHE_WAYS = CONSTANTS["ZC_EVALCACHE_WAYS"]
# ZC_EVALCACHE_STAT_* in their order: the merged calls' five int64 counters, the plain calls' first four
EVALCACHE_MERGED_STATS = tuple(k[len("ZC_EVALCACHE_STAT_"):].lower() for k in sorted(
    (k for k in CONSTANTS if k.startswith("ZC_EVALCACHE_STAT_")), key=CONSTANTS.get))
EVALCACHE_STATS = EVALCACHE_MERGED_STATS[:CONSTANTS["ZC_EVALCACHE_STAT_MERGED"]]


def evalcache_check_sizes(entries: int, key_bytes: int, logit_bytes: int):
    """What zc_evalcache_bytes checks, with the reason (the library records no message)."""
    if not 1 <= int(entries) <= 1 << 30:
        raise ValueError(f"entries must be in [1, 2^30] (got {entries})")
    if key_bytes < 8 or key_bytes % 8 or key_bytes > 512:
        raise ValueError(f"key_bytes must be a multiple of 8 in [8, 512] (got {key_bytes})")
    if logit_bytes < 0 or logit_bytes % 2 or logit_bytes > 1 << 20:
        raise ValueError(f"logit_bytes must be even, in [0, 2^20] (got {logit_bytes})")


def evalcache_bytes(entries: int, key_bytes: int, logit_bytes: int) -> tuple[int, int]:
    """zc_evalcache_bytes: (the table's size in bytes, its number of sets)."""
    evalcache_check_sizes(entries, key_bytes, logit_bytes)
    b, s = ctypes.c_int64(0), ctypes.c_int64(0)
    _arena_rc("zc_evalcache_bytes", lib().zc_evalcache_bytes(int(entries), int(key_bytes), int(logit_bytes),
                                                             ctypes.byref(b), ctypes.byref(s)))
    return b.value, s.value


def evalcache_clear(d_table: int, entries: int, key_bytes: int, logit_bytes: int, stream: int = 0):
    """zc_evalcache_clear_async: empties the table.  Only enqueues."""
    _arena_rc("zc_evalcache_clear_async", lib().zc_evalcache_clear_async(
        ctypes.c_void_p(d_table), int(entries), int(key_bytes), int(logit_bytes), ctypes.c_void_p(stream or None)))


def _evalcache_flush(name: str, n_rows: int, rows_per_game: int, game_rows: int, plane_bytes, d_count: int,
                     needed: tuple, args: tuple, apart: tuple = ()):
    """What the six flush wrappers share: the checks of the rows, of plane_bytes (None: a commit has
    none) and of the pointers (d_count always, `needed` in a flush of rows; `apart`: two that must
    differ), then the call of entry point `name` with args, integers and device pointers alike."""
    if n_rows < 0 or not 1 <= rows_per_game <= game_rows or n_rows % rows_per_game:
        raise ValueError(f"{name}: need 1 <= rows_per_game <= game_rows and n_rows a multiple of rows_per_game "
                         f"(got n_rows {n_rows}, rows_per_game {rows_per_game}, game_rows {game_rows})")
    if n_rows // rows_per_game * game_rows >= 1 << 31:
        raise ValueError(f"{name}: the buffers' rows must number below 2^31")
    if plane_bytes is not None and (plane_bytes < 2 or plane_bytes % 2):
        raise ValueError(f"{name}: plane_bytes must be a positive multiple of 2 (got {plane_bytes})")
    if not d_count or (n_rows and not all(needed)):
        raise ValueError(f"{name}: null device pointer")
    if n_rows and apart and apart[0] == apart[1]:
        raise ValueError(f"{name}: the two networks' dense planes must be two buffers")
    _arena_rc(name, getattr(lib(), name)(*(int(a or 0) for a in args)))


def evalcache_probe(d_table: int, entries: int, key_bytes: int, logit_bytes: int, n_rows: int, rows_per_game: int,
                    game_rows: int, d_keys: int, d_planes: int, plane_bytes: int, d_out_values: int, d_out_logits: int,
                    d_dense_planes: int, d_miss_rows: int, d_count: int, d_stats: int = 0, stream: int = 0):
    """zc_evalcache_probe_async (include/zeroclone.h) on device pointers.  Only enqueues."""
    _evalcache_flush("zc_evalcache_probe_async", n_rows, rows_per_game, game_rows, plane_bytes, d_count,
                     (d_keys, d_planes, d_out_values, d_dense_planes, d_miss_rows, d_out_logits or not logit_bytes),
                     (d_table, entries, key_bytes, logit_bytes, n_rows, rows_per_game, game_rows, d_keys, d_planes,
                      plane_bytes, d_out_values, d_out_logits, d_dense_planes, d_miss_rows, d_count, d_stats, stream))


def evalcache_commit(d_table: int, entries: int, key_bytes: int, logit_bytes: int, n_rows: int, rows_per_game: int,
                     game_rows: int, d_keys: int, d_miss_rows: int, d_count: int, d_dense_values: int,
                     d_dense_logits: int, d_out_values: int, d_out_logits: int, d_stats: int = 0, stream: int = 0):
    """zc_evalcache_commit_async (include/zeroclone.h) on device pointers; leaves *d_count = 0.
    Only enqueues."""
    _evalcache_flush("zc_evalcache_commit_async", n_rows, rows_per_game, game_rows, None, d_count,
                     (d_keys, d_miss_rows, d_dense_values, d_out_values,
                      (d_dense_logits and d_out_logits) or not logit_bytes),
                     (d_table, entries, key_bytes, logit_bytes, n_rows, rows_per_game, game_rows, d_keys, d_miss_rows,
                      d_count, d_dense_values, d_dense_logits, d_out_values, d_out_logits, d_stats, stream))


def evalcache_check_merged_sizes(entries: int, key_bytes: int, logit_bytes: int):
    """evalcache_check_sizes for the merged calls: entries 0 is "no table"."""
    evalcache_check_sizes(entries or EVALCACHE_WAYS, key_bytes, logit_bytes)


def evalcache_merge_scratch_bytes(n_rows: int) -> int:
    """zc_evalcache_merge_scratch_bytes: the flush-local scratch of the merged calls, in bytes."""
    if not 0 <= n_rows < 1 << 31:
        raise ValueError(f"n_rows must be in [0, 2^31) (got {n_rows})")
    b = ctypes.c_int64(0)
    _arena_rc("zc_evalcache_merge_scratch_bytes", lib().zc_evalcache_merge_scratch_bytes(int(n_rows), ctypes.byref(b)))
    return b.value


def evalcache_probe_merged(d_table: int, entries: int, key_bytes: int, logit_bytes: int, n_rows: int,
                           rows_per_game: int, game_rows: int, d_keys: int, d_planes: int, plane_bytes: int,
                           d_out_values: int, d_out_logits: int, d_dense_planes: int, d_miss_rows: int, d_count: int,
                           d_stats: int, d_scratch: int, stream: int = 0):
    """zc_evalcache_probe_merged_async (include/zeroclone.h) on device pointers; d_table 0 with
    entries 0: no table.  Only enqueues."""
    _evalcache_flush("zc_evalcache_probe_merged_async", n_rows, rows_per_game, game_rows, plane_bytes, d_count,
                     (d_keys, d_planes, d_out_values, d_dense_planes, d_miss_rows, d_scratch,
                      d_out_logits or not logit_bytes),
                     (d_table, entries, key_bytes, logit_bytes, n_rows, rows_per_game, game_rows, d_keys, d_planes,
                      plane_bytes, d_out_values, d_out_logits, d_dense_planes, d_miss_rows, d_count, d_stats, d_scratch,
                      stream))


def evalcache_commit_merged(d_table: int, entries: int, key_bytes: int, logit_bytes: int, n_rows: int,
                            rows_per_game: int, game_rows: int, d_keys: int, d_miss_rows: int, d_count: int,
                            d_dense_values: int, d_dense_logits: int, d_out_values: int, d_out_logits: int,
                            d_stats: int, d_scratch: int, stream: int = 0):
    """zc_evalcache_commit_merged_async (include/zeroclone.h) on device pointers; leaves *d_count
    = 0 and the scratch ready for the next flush.  Only enqueues."""
    _evalcache_flush("zc_evalcache_commit_merged_async", n_rows, rows_per_game, game_rows, None, d_count,
                     (d_keys, d_miss_rows, d_dense_values, d_out_values, d_scratch,
                      (d_dense_logits and d_out_logits) or not logit_bytes),
                     (d_table, entries, key_bytes, logit_bytes, n_rows, rows_per_game, game_rows, d_keys, d_miss_rows,
                      d_count, d_dense_values, d_dense_logits, d_out_values, d_out_logits, d_stats, d_scratch, stream))


def _evalcache_routed_tables(name: str, d_table_a: int, d_table_b: int, entries: int, key_bytes: int,
                             logit_bytes: int):
    evalcache_check_merged_sizes(entries, key_bytes, logit_bytes)
    if bool(d_table_a) != bool(d_table_b) or bool(d_table_a) != bool(entries) or (d_table_a and d_table_a == d_table_b):
        raise ValueError(f"{name}: need two different tables of `entries` entries, or none with entries 0")


def evalcache_probe_routed(d_table_a: int, d_table_b: int, entries: int, key_bytes: int, logit_bytes: int, n_rows: int,
                           rows_per_game: int, game_rows: int, d_route: int, d_keys: int, d_planes: int,
                           plane_bytes: int, d_out_values: int, d_out_logits: int, d_dense_planes_a: int,
                           d_dense_planes_b: int, d_miss_rows: int, d_count: int, d_stats: int = 0,
                           d_scratch: int = 0, stream: int = 0):
    """zc_evalcache_probe_routed_async (include/zeroclone.h) on device pointers: d_miss_rows
    [2][n_rows], d_count [2], d_stats [2][5]; both tables 0 with entries 0: no tables; d_scratch 0:
    no merging.  Only enqueues."""
    name = "zc_evalcache_probe_routed_async"
    _evalcache_routed_tables(name, d_table_a, d_table_b, entries, key_bytes, logit_bytes)
    _evalcache_flush(name, n_rows, rows_per_game, game_rows, plane_bytes, d_count,
                     (d_route, d_keys, d_planes, d_out_values, d_dense_planes_a, d_dense_planes_b, d_miss_rows,
                      d_out_logits or not logit_bytes),
                     (d_table_a, d_table_b, entries, key_bytes, logit_bytes, n_rows, rows_per_game, game_rows, d_route,
                      d_keys, d_planes, plane_bytes, d_out_values, d_out_logits, d_dense_planes_a, d_dense_planes_b,
                      d_miss_rows, d_count, d_stats, d_scratch, stream),
                     apart=(d_dense_planes_a, d_dense_planes_b))


def evalcache_commit_routed(d_table_a: int, d_table_b: int, entries: int, key_bytes: int, logit_bytes: int,
                            n_rows: int, rows_per_game: int, game_rows: int, d_keys: int, d_miss_rows: int,
                            d_count: int, d_dense_values_a: int, d_dense_logits_a: int, d_dense_values_b: int,
                            d_dense_logits_b: int, d_out_values: int, d_out_logits: int, d_stats: int = 0,
                            d_scratch: int = 0, stream: int = 0):
    """zc_evalcache_commit_routed_async (include/zeroclone.h) on device pointers; leaves both counts
    0 and the scratch ready for the next flush.  Only enqueues."""
    name = "zc_evalcache_commit_routed_async"
    _evalcache_routed_tables(name, d_table_a, d_table_b, entries, key_bytes, logit_bytes)
    _evalcache_flush(name, n_rows, rows_per_game, game_rows, None, d_count,
                     (d_keys, d_miss_rows, d_dense_values_a, d_dense_values_b, d_out_values,
                      (d_dense_logits_a and d_dense_logits_b and d_out_logits) or not logit_bytes),
                     (d_table_a, d_table_b, entries, key_bytes, logit_bytes, n_rows, rows_per_game, game_rows, d_keys,
                      d_miss_rows, d_count, d_dense_values_a, d_dense_logits_a, d_dense_values_b, d_dense_logits_b,
                      d_out_values, d_out_logits, d_stats, d_scratch, stream))


def _train_rc(name: str, rc: int):
    """The training entry points record no message either: the wrappers below check what the
    library checks."""
    if rc == ZC_EINVAL:
        raise ValueError(f"{name}: bad argument")
    if rc < 0:
        raise ZeroCloneError(rc, f"{name}: the launch failed")


def train_batch(ts: TrainSet, B: int, d_index: int, d_flags: int, planes_f16: bool, d_planes: int, d_z: int,
                d_legal: int, d_n_legal: int, d_target: int, d_status: int, stream: int = 0):
    """zc_train_batch_async on device pointers: batch row b = set row d_index[b] decoded to planes,
    label, legal moves and targets.  d_flags 0: no mirror flags.  Only enqueues."""
    if B < 0:
        raise ValueError(f"B must be >= 0 (got {B})")
    if (ts.game, ts.row_bytes) not in ((ZC_TRAIN_C4, 24), (ZC_TRAIN_CHESS, 72)):
        raise ValueError(f"zc_train_batch_async: game {ts.game} with rows of {ts.row_bytes} bytes")
    if ts.game == ZC_TRAIN_CHESS and d_flags:
        raise ValueError("zc_train_batch_async: a chess position has no mirror image (flags must be None)")
    if bool(ts.d_pi_off) != bool(ts.d_pi):
        raise ValueError("zc_train_batch_async: d_pi_off and d_pi go together")
    if B and not (ts.d_rows and ts.d_labels and d_index and d_planes and d_z and d_legal and d_n_legal and d_target
                  and d_status):
        raise ValueError("zc_train_batch_async: null device pointer")
    _train_rc("zc_train_batch_async", lib().zc_train_batch_async(
        ctypes.byref(ts), int(B), ctypes.c_void_p(d_index), ctypes.c_void_p(d_flags or None),
        ZC_F16 if planes_f16 else ZC_F32, ctypes.c_void_p(d_planes), ctypes.c_void_p(d_z), ctypes.c_void_p(d_legal),
        ctypes.c_void_p(d_n_legal), ctypes.c_void_p(d_target), ctypes.c_void_p(d_status),
        ctypes.c_void_p(stream or None)))


def train_loss_scratch_bytes(B: int) -> int:
    need = ctypes.c_int64(0)
    _train_rc("zc_train_loss_scratch_bytes", lib().zc_train_loss_scratch_bytes(int(B), ctypes.byref(need)))
    return need.value


def train_loss(B: int, width: int, stride: int, d_logits: int, logits_f16: bool, d_v: int, d_z: int, d_legal: int,
               d_n_legal: int, d_target: int, d_scratch: int, scratch_bytes: int, d_loss: int, d_grad_v: int,
               d_grad_logits: int, stream: int = 0):
    """zc_train_loss_async on device pointers: d_loss[2] = {Lv, Lp}, d_grad_v [B], d_grad_logits
    [B, width] (written in full).  d_logits 0: a value-only model.  Only enqueues."""
    if B < 1:
        raise ValueError(f"B must be >= 1 (got {B})")
    if not (d_v and d_z and d_loss and d_grad_v):
        raise ValueError("zc_train_loss_async: null device pointer")
    if not d_scratch or d_scratch & 15 or scratch_bytes < (6 * B + 4) * 4:
        raise ValueError(f"zc_train_loss_async: scratch of {scratch_bytes} bytes, need {(6 * B + 4) * 4} 16-byte aligned")
    if d_logits:
        if width not in (7, 4096):
            raise ValueError(f"width must be 7 or 4096 (got {width})")
        if not 1 <= stride <= (64 if width == 7 else CHESS_MAX_MOVES):
            raise ValueError(f"stride {stride} out of range for width {width}")
        if not (d_legal and d_n_legal and d_target and d_grad_logits):
            raise ValueError("zc_train_loss_async: null device pointer")
        if width == 4096 and d_grad_logits & 15:
            raise ValueError("zc_train_loss_async: grad_logits must be 16-byte aligned")
    _train_rc("zc_train_loss_async", lib().zc_train_loss_async(
        int(B), int(width), int(stride), ctypes.c_void_p(d_logits or None), ZC_F16 if logits_f16 else ZC_F32,
        ctypes.c_void_p(d_v), ctypes.c_void_p(d_z), ctypes.c_void_p(d_legal or None), ctypes.c_void_p(d_n_legal or None),
        ctypes.c_void_p(d_target or None), ctypes.c_void_p(d_scratch), int(scratch_bytes), ctypes.c_void_p(d_loss),
        ctypes.c_void_p(d_grad_v), ctypes.c_void_p(d_grad_logits or None), ctypes.c_void_p(stream or None)))


# ---- the stepwise protocol's wrappers, each written once and bound by NativeEngine under both
# games' names: g is the game's entry points (_C4 or _CHESS), fn one of them.  Device pointers as
# ints, 0 = NULL.
def _ext_begin(fn, self, first_game, n, d_roots, sims, c, batch_size, extra, stream):
    """Both games' ext_begin; extra: what the game's entry point takes after batch_size."""
    check(fn(self._h, first_game, n, ctypes.c_void_p(d_roots), int(sims), float(c), int(batch_size), *extra,
             ctypes.c_void_p(stream or None)))


def _select(fn, self, first_game, n, flush, d_leaves, d_planes, planes_dtype, d_counts, stream):
    """Every select, of the value and the PUCT searches; planes_dtype: a ZC_F* code."""
    check(fn(self._h, first_game, n, int(flush), ctypes.c_void_p(d_leaves or None), ctypes.c_void_p(d_planes or None),
             planes_dtype, ctypes.c_void_p(d_counts or None), ctypes.c_void_p(stream or None)))


def _ext_select(g):
    def ext_select(self, first_game: int, n: int, flush: int, d_leaves: int = 0, d_planes: int = 0,
                   planes_f16: bool = True, d_counts: int = 0, stream: int = 0) -> None:
        _select(g.ext_select, self, first_game, n, flush, d_leaves, d_planes, ZC_F16 if planes_f16 else ZC_F32,
                d_counts, stream)
    return ext_select


def _ext_backup(g):
    def ext_backup(self, first_game: int, n: int, flush: int, d_values: int, stream: int = 0) -> None:
        check(g.ext_backup(self._h, first_game, n, int(flush), ctypes.c_void_p(d_values),
                           ctypes.c_void_p(stream or None)))
    return ext_backup


def _ext_end(g):
    def ext_end(self, first_game: int, n: int, d_move: int, d_na: int, d_stats: int, stream: int = 0) -> None:
        check(g.ext_end(self._h, first_game, n, ctypes.c_void_p(d_move), ctypes.c_void_p(d_na),
                        ctypes.c_void_p(d_stats), ctypes.c_void_p(stream or None)))
    return ext_end


def _hp_walk(g):
    def hp_walk(self, game: int, flush: int, leaf: int, d_node: int, stream: int = 0) -> None:
        check(g.hp_walk(self._h, game, int(flush), int(leaf), ctypes.c_void_p(d_node), ctypes.c_void_p(stream or None)))
    return hp_walk


def _hp_expand(g):
    def hp_expand(self, game: int, flush: int, leaf: int, index: int, d_leaf: int = 0, stream: int = 0) -> None:
        """index: into the walk's untried moves, the range the game's entry point checks (7
        columns, ZC_CHESS_MAX_MOVES moves); -1 at a node without untried moves."""
        check(g.hp_expand(self._h, game, int(flush), int(leaf), int(index), ctypes.c_void_p(d_leaf or None),
                          ctypes.c_void_p(stream or None)))
    return hp_expand


def _puct_begin(g):
    def puct_begin(self, first_game, n, d_roots, sims, c_puct, batch_size, alpha, eps, seed, d_search_no=0, stream=0):
        check(g.puct_begin(self._h, first_game, n, ctypes.c_void_p(d_roots), int(sims), float(c_puct),
                           int(batch_size), float(alpha), float(eps), int(seed) & (2**64 - 1),
                           ctypes.c_void_p(d_search_no or None), ctypes.c_void_p(stream or None)))
    return puct_begin


def _puct_begin_reuse(g):
    def puct_begin_reuse(self, first_game, n, d_roots, sims, c_puct, batch_size, alpha, eps, seed, d_search_no=0,
                         d_kept=0, stream=0):
        """puct_begin that keeps each game's subtree of its new root (zc_*_puct_begin_reuse)."""
        check(g.puct_begin_reuse(self._h, first_game, n, ctypes.c_void_p(d_roots), int(sims), float(c_puct),
                                 int(batch_size), float(alpha), float(eps), int(seed) & (2**64 - 1),
                                 ctypes.c_void_p(d_search_no or None), ctypes.c_void_p(d_kept or None),
                                 ctypes.c_void_p(stream or None)))
    return puct_begin_reuse


def _puct_forget(g):
    def puct_forget(self, first_game, n, stream=0):
        check(g.puct_forget(self._h, first_game, n, ctypes.c_void_p(stream or None)))
    return puct_forget


def _puct_forget_fresh(g):
    def puct_forget_fresh(self, first_game, n, d_slot, stream=0):
        check(g.puct_forget_fresh(self._h, first_game, n, ctypes.c_void_p(d_slot), ctypes.c_void_p(stream or None)))
    return puct_forget_fresh


def _puct_backup(g):
    def puct_backup(self, first_game, n, flush, d_values, d_logits, logits_f16=False, stream=0, rows=0):
        """rows: values / logits rows per game (0: batch_size; flush 0 also takes 1 — the roots alone)."""
        check(g.puct_backup_ex(self._h, first_game, n, int(flush), ctypes.c_void_p(d_values),
                               ctypes.c_void_p(d_logits), ZC_F16 if logits_f16 else ZC_F32, int(rows),
                               ctypes.c_void_p(stream or None)))
    return puct_backup


def _puct_end(g):
    def puct_end(self, first_game, n, temperature, d_move, d_na, d_prior, d_stats, stream=0):
        check(g.puct_end(self._h, first_game, n, float(temperature), ctypes.c_void_p(d_move), ctypes.c_void_p(d_na),
                         ctypes.c_void_p(d_prior or None), ctypes.c_void_p(d_stats), ctypes.c_void_p(stream or None)))
    return puct_end


class NativeEngine:
    """One HIP device's arena: `max_games` resident games, trees of max_sims+1 nodes."""

    def __init__(self, max_games: int, max_sims: int, max_batch: int = 32, device: int = 0):
        L = lib()
        cfg = EngineConfig(device, max_games, max_sims, max_batch)
        h = ctypes.c_void_p()
        check(L.zc_engine_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.max_games, self.max_sims, self.max_batch, self.device = max_games, max_sims, max_batch, device

    def close(self):
        if getattr(self, "_h", None):
            lib().zc_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def footprint(self) -> int:
        b = ctypes.c_int64(0)
        check(lib().zc_engine_footprint(self._h, ctypes.byref(b)))
        return b.value

    # ---- random streams
    def seed(self, first_game: int, seeds) -> None:
        s = np.ascontiguousarray(seeds, dtype=np.uint64)
        check(lib().zc_rng_seed(self._h, first_game, len(s), s.ctypes.data_as(P(ctypes.c_uint64))))

    def set_rng_state(self, game: int, mt624, index: int) -> None:
        mt = np.ascontiguousarray(mt624, dtype=np.uint32)
        assert mt.shape == (624,)
        check(lib().zc_rng_set_state(self._h, game, mt.ctypes.data_as(P(ctypes.c_uint32)), int(index)))

    def get_rng_state(self, game: int):
        mt = np.zeros(624, np.uint32)
        idx = ctypes.c_int32(0)
        check(lib().zc_rng_get_state(self._h, game, mt.ctypes.data_as(P(ctypes.c_uint32)), ctypes.byref(idx)))
        return mt, idx.value

    # ---- search
    def c4_search(self, roots: np.ndarray, sims: int, c: float = 1.4, batch_size: int = 32, first_game: int = 0):
        roots = np.ascontiguousarray(roots, dtype=C4_STATE_DTYPE)
        n = roots.shape[0]
        mv = np.zeros(n, np.int32)
        na = np.zeros((n, 7), np.int32)
        st = np.zeros(n, STATS_DTYPE)
        check(lib().zc_c4_search(self._h, first_game, n, _ptr(roots), int(sims), float(c), int(batch_size),
                                 _ptr(mv), _ptr(na), _ptr(st)))
        return mv, na, st

    def c4_search_games(self, games, roots: np.ndarray, sims: int, c: float = 1.4, batch_size: int = 32):
        ids = np.ascontiguousarray(games, dtype=np.int32)
        roots = np.ascontiguousarray(roots, dtype=C4_STATE_DTYPE)
        n = roots.shape[0]
        assert ids.shape == (n,)
        mv = np.zeros(n, np.int32)
        na = np.zeros((n, 7), np.int32)
        st = np.zeros(n, STATS_DTYPE)
        check(lib().zc_c4_search_games(self._h, n, _ptr(ids), _ptr(roots), int(sims), float(c), int(batch_size),
                                       _ptr(mv), _ptr(na), _ptr(st)))
        return mv, na, st

    def c4_rollout_mode(self, mode: str = "exact", seed: int = 0) -> None:
        """"exact" (the game's MT19937 stream, bit-identical to the reference) or "philox"
        (leaf-parallel rollouts on per-leaf counter-based streams; statistical parity only)."""
        m = {"exact": ROLLOUT_EXACT, "philox": ROLLOUT_PHILOX}[mode]
        check(lib().zc_c4_set_rollout_mode(self._h, m, int(seed) & (2**64 - 1)))

    def c4_search_async(self, d_roots: int, n: int, sims: int, c: float, batch_size: int, d_move: int, d_na: int,
                        d_stats: int, stream: int = 0, first_game: int = 0) -> None:
        """Device-pointer entry (ints from torch .data_ptr()); enqueued on `stream`."""
        check(lib().zc_c4_search_async(self._h, first_game, n, ctypes.c_void_p(d_roots), int(sims), float(c),
                                       int(batch_size), ctypes.c_void_p(d_move), ctypes.c_void_p(d_na),
                                       ctypes.c_void_p(d_stats), ctypes.c_void_p(stream or None)))

    def c4_selfplay_async(self, d_roots: int, n: int, sims: int, c: float, batch_size: int, moves: int,
                          d_states: int, d_moves16: int, d_results: int, d_stats: int, stream: int = 0,
                          first_game: int = 0) -> None:
        """`moves` self-play moves per game in one launch (zc_c4_selfplay_async)."""
        check(lib().zc_c4_selfplay_async(self._h, first_game, n, ctypes.c_void_p(d_roots), int(sims), float(c),
                                         int(batch_size), int(moves), ctypes.c_void_p(d_states),
                                         ctypes.c_void_p(d_moves16), ctypes.c_void_p(d_results),
                                         ctypes.c_void_p(d_stats), ctypes.c_void_p(stream or None)))

    def c4_selfplay_pooled_async(self, d_roots: int, n: int, sims: int, c: float, batch_size: int, moves_cap: int,
                                 budget: int, d_ticket: int, d_states: int, d_moves16: int, d_results: int,
                                 d_stats: int, stream: int = 0, first_game: int = 0, carry: bool = False) -> None:
        """`budget` self-play moves shared by the games in one launch, at most `moves_cap` per
        game (zc_c4_selfplay_pooled_async; carry: in-flight moves carry over into the next
        launch, zc_c4_selfplay_carry_async)."""
        fn = lib().zc_c4_selfplay_carry_async if carry else lib().zc_c4_selfplay_pooled_async
        check(fn(self._h, first_game, n, ctypes.c_void_p(d_roots), int(sims),
                                                float(c), int(batch_size), int(moves_cap), int(budget),
                                                ctypes.c_void_p(d_ticket), ctypes.c_void_p(d_states),
                                                ctypes.c_void_p(d_moves16), ctypes.c_void_p(d_results),
                                                ctypes.c_void_p(d_stats), ctypes.c_void_p(stream or None)))

    def c4_selfplay_visits(self, d_na: int | None, steps_cap: int = 0) -> None:
        """The self-play launches' per-step visit-count staging [steps_cap][n][7] int32
        (zc_c4_selfplay_visits; None: off)."""
        check(lib().zc_c4_selfplay_visits(self._h, ctypes.c_void_p(d_na or None), int(steps_cap)))

    def chess_selfplay_visits(self, d_na: int | None, d_root_moves: int | None = None, steps_cap: int = 0) -> None:
        """The chess self-play launches' staging of visit counts and root moves
        [steps_cap][n][CHESS_MAX_MOVES] (zc_chess_selfplay_visits; None: off)."""
        check(lib().zc_chess_selfplay_visits(self._h, ctypes.c_void_p(d_na or None),
                                             ctypes.c_void_p(d_root_moves or None), int(steps_cap)))

    def c4_carry_discard(self, first_game: int, n: int, stream: int = 0) -> None:
        check(lib().zc_c4_carry_discard(self._h, int(first_game), int(n), ctypes.c_void_p(stream or None)))

    def c4_pooled_max_games(self, batch_size: int) -> int:
        n = ctypes.c_int32(0)
        check(lib().zc_c4_pooled_max_games(self._h, int(batch_size), ctypes.byref(n)))
        return n.value

    # ---- any game backend (zc_gen_*)
    def gen_reserve(self, nodes: int, slots: int) -> None:
        check(lib().zc_gen_reserve(self._h, int(nodes), int(slots)))

    def gen_capacity(self):
        n, s = ctypes.c_int32(0), ctypes.c_int64(0)
        check(lib().zc_gen_capacity(self._h, ctypes.byref(n), ctypes.byref(s)))
        return n.value, s.value

    def gen_begin(self, sims: int, c: float, batch_size: int, root_moves: int, stream: int = 0) -> None:
        check(lib().zc_gen_begin(self._h, int(sims), float(c), int(batch_size), int(root_moves),
                                 ctypes.c_void_p(stream or None)))

    def gen_walk(self, d_out: int, out_cap: int, stream: int = 0) -> None:
        check(lib().zc_gen_walk(self._h, ctypes.c_void_p(d_out), int(out_cap), ctypes.c_void_p(stream or None)))

    def gen_expand(self, untried_index: int, child_moves: int, stream: int = 0) -> None:
        check(lib().zc_gen_expand(self._h, int(untried_index), int(child_moves), ctypes.c_void_p(stream or None)))

    def gen_backup(self, n: int, d_values: int, stream: int = 0) -> None:
        check(lib().zc_gen_backup(self._h, int(n), ctypes.c_void_p(d_values), ctypes.c_void_p(stream or None)))

    def gen_end(self, d_out: int, d_root_na: int = 0, na_cap: int = 0, stream: int = 0) -> None:
        check(lib().zc_gen_end(self._h, ctypes.c_void_p(d_out), ctypes.c_void_p(d_root_na or None), int(na_cap),
                               ctypes.c_void_p(stream or None)))

    def c4_play_async(self, d_states: int, n: int, d_moves: int, d_results: int, reset: bool = True,
                      stream: int = 0) -> None:
        check(lib().zc_c4_play_async(self._h, n, ctypes.c_void_p(d_states), ctypes.c_void_p(d_moves),
                                     ctypes.c_void_p(d_results), int(bool(reset)), ctypes.c_void_p(stream or None)))

    # ---- stepwise value search (caller-supplied values), with the host-policy walk and expansion
    def c4_ext_begin(self, first_game: int, n: int, d_roots: int, sims: int, c: float, batch_size: int,
                     stream: int = 0) -> None:
        _ext_begin(_C4.ext_begin, self, first_game, n, d_roots, sims, c, batch_size, (), stream)

    def chess_ext_begin(self, first_game: int, n: int, d_roots: int, sims: int, c: float, batch_size: int,
                        policy: int = 0, freedom: float = 0.0, stream: int = 0):
        _ext_begin(_CHESS.ext_begin, self, first_game, n, d_roots, sims, c, batch_size, (int(policy), float(freedom)),
                   stream)

    c4_ext_select, chess_ext_select = _ext_select(_C4), _ext_select(_CHESS)
    c4_ext_backup, chess_ext_backup = _ext_backup(_C4), _ext_backup(_CHESS)
    c4_ext_end, chess_ext_end = _ext_end(_C4), _ext_end(_CHESS)
    c4_hp_walk, chess_hp_walk = _hp_walk(_C4), _hp_walk(_CHESS)
    c4_hp_expand, chess_hp_expand = _hp_expand(_C4), _hp_expand(_CHESS)

    # ---- stepwise PUCT search
    c4_puct_begin, chess_puct_begin = _puct_begin(_C4), _puct_begin(_CHESS)
    c4_puct_begin_reuse, chess_puct_begin_reuse = _puct_begin_reuse(_C4), _puct_begin_reuse(_CHESS)
    c4_puct_forget, chess_puct_forget = _puct_forget(_C4), _puct_forget(_CHESS)
    c4_puct_forget_fresh, chess_puct_forget_fresh = _puct_forget_fresh(_C4), _puct_forget_fresh(_CHESS)
    c4_puct_backup, chess_puct_backup = _puct_backup(_C4), _puct_backup(_CHESS)
    c4_puct_end, chess_puct_end = _puct_end(_C4), _puct_end(_CHESS)

    def c4_puct_select(self, first_game, n, flush, d_leaves=0, d_planes=0, planes_f16=True, d_counts=0, stream=0):
        _select(_C4.puct_select, self, first_game, n, flush, d_leaves, d_planes, ZC_F16 if planes_f16 else ZC_F32,
                d_counts, stream)

    def chess_puct_select(self, first_game, n, flush, d_leaves=0, d_planes=0, planes_f16=True, d_counts=0, stream=0,
                          planes_nhwc=False):
        """planes_nhwc: fp16 planes in the tower's input layout [n*bs][64][32] (ZC_F16_NHWC32)."""
        _select(_CHESS.puct_select, self, first_game, n, flush, d_leaves, d_planes,
                ZC_F16_NHWC32 if planes_nhwc else ZC_F16 if planes_f16 else ZC_F32, d_counts, stream)

    # ---- chess rules (device pointers; stream 0 = null stream)
    def chess_legal_moves_async(self, n: int, d_states: int, d_moves: int, d_counts: int, stream: int = 0):
        check(lib().zc_chess_legal_moves_async(self._h, n, ctypes.c_void_p(d_states), ctypes.c_void_p(d_moves),
                                               ctypes.c_void_p(d_counts), ctypes.c_void_p(stream or None)))

    def chess_children_async(self, n: int, d_states: int, d_children: int, d_moves: int, d_counts: int,
                             stream: int = 0):
        check(lib().zc_chess_children_async(self._h, n, ctypes.c_void_p(d_states), ctypes.c_void_p(d_children),
                                            ctypes.c_void_p(d_moves or None), ctypes.c_void_p(d_counts),
                                            ctypes.c_void_p(stream or None)))

    def debug_chess_tree(self, game: int, max_nodes: int = 1 << 16, max_slots: int = 1 << 22) -> dict:
        """Game `game`'s chess tree after a search (test hook): node records and slot arrays."""
        nodes = np.zeros(max_nodes, CHESS_NODE_DTYPE)
        mv = np.zeros(max_slots, np.uint16)
        pr = np.zeros(max_slots, np.float32)
        na = np.zeros(max_slots, np.int32)
        w = np.zeros(max_slots, np.float64)
        ch = np.zeros(max_slots, np.uint16)
        cnt = np.zeros(2, np.int32)
        check(lib().zc_debug_chess_tree(self._h, int(game), max_nodes, max_slots, _ptr(nodes), _ptr(mv), _ptr(pr),
                                        _ptr(na), _ptr(w), _ptr(ch), _ptr(cnt)))
        n, s = int(cnt[0]), int(cnt[1])
        return {"nodes": nodes[:n], "mv": mv[:s], "prior": pr[:s], "na": na[:s], "w": w[:s], "child": ch[:s]}

    def chess_play_async(self, n: int, d_in: int, d_moves: int, d_out: int, stream: int = 0):
        check(lib().zc_chess_play_async(self._h, n, ctypes.c_void_p(d_in), ctypes.c_void_p(d_moves),
                                        ctypes.c_void_p(d_out), ctypes.c_void_p(stream or None)))

    def debug_chess_probe_async(self, n: int, d_states: int, d_out: int, stream: int = 0):
        """zc_debug_chess_probe_async: -2 (a legal move proven, no list) or the list length."""
        check(lib().zc_debug_chess_probe_async(self._h, n, ctypes.c_void_p(d_states), ctypes.c_void_p(d_out),
                                               ctypes.c_void_p(stream or None)))

    def chess_terminal_async(self, n: int, d_states: int, d_flags: int, stream: int = 0):
        check(lib().zc_chess_terminal_async(self._h, n, ctypes.c_void_p(d_states), ctypes.c_void_p(d_flags),
                                            ctypes.c_void_p(stream or None)))

    def chess_planes_async(self, n: int, d_states: int, d_planes: int, f16: bool = False, stream: int = 0):
        check(lib().zc_chess_planes_async(self._h, n, ctypes.c_void_p(d_states), ctypes.c_void_p(d_planes),
                                          ZC_F16 if f16 else ZC_F32, ctypes.c_void_p(stream or None)))

    # ---- chess tree search (device pointers)
    def chess_reserve(self):
        check(lib().zc_chess_reserve(self._h))

    def chess_search_async(self, first_game: int, n: int, d_roots: int, sims: int, c: float, batch_size: int,
                           policy: int, freedom: float, d_move: int, d_na: int, d_stats: int, stream: int = 0):
        check(lib().zc_chess_search_async(self._h, first_game, n, ctypes.c_void_p(d_roots), int(sims), float(c),
                                          int(batch_size), int(policy), float(freedom), ctypes.c_void_p(d_move),
                                          ctypes.c_void_p(d_na), ctypes.c_void_p(d_stats),
                                          ctypes.c_void_p(stream or None)))

    # ---- the walk diagnostic (device pointers; tools/prof_walk.py)
    def c4_walk_async(self, first_game: int, n: int, d_roots: int, sims: int, c: float, batch_size: int, mode: int,
                      d_vals: int, d_words: int, d_move: int, d_na: int, d_stats: int, stream: int = 0):
        check(lib().zc_debug_c4_walk_async(self._h, first_game, n, ctypes.c_void_p(d_roots), int(sims), float(c),
                                           int(batch_size), int(mode), ctypes.c_void_p(d_vals),
                                           ctypes.c_void_p(d_words), ctypes.c_void_p(d_move), ctypes.c_void_p(d_na),
                                           ctypes.c_void_p(d_stats), ctypes.c_void_p(stream or None)))

    def rng_copy(self, first_game: int, n: int, d_buf: int, restore: bool, stream: int = 0):
        check(lib().zc_debug_rng_copy(self._h, first_game, n, ctypes.c_void_p(d_buf), 1 if restore else 0,
                                      ctypes.c_void_p(stream or None)))

    # ---- Value('random_rollout') on chess (device pointers)
    def chess_rollouts_async(self, game: int, n: int, d_states: int, d_hist: int, d_hist_len: int, hist_cap: int,
                             d_values: int, d_status: int = 0, stream: int = 0):
        check(lib().zc_chess_rollouts_async(self._h, int(game), int(n), ctypes.c_void_p(d_states),
                                            ctypes.c_void_p(d_hist), ctypes.c_void_p(d_hist_len), int(hist_cap),
                                            ctypes.c_void_p(d_values), ctypes.c_void_p(d_status or None),
                                            ctypes.c_void_p(stream or None)))

    def chess_ext_rollouts(self, first_game: int, n: int, flush: int, d_hist: int, d_hist_len: int, hist_cap: int,
                           d_values: int, d_status: int = 0, stream: int = 0):
        check(_CHESS.ext_rollouts(self._h, first_game, n, int(flush), ctypes.c_void_p(d_hist),
                                  ctypes.c_void_p(d_hist_len), int(hist_cap), ctypes.c_void_p(d_values),
                                  ctypes.c_void_p(d_status or None), ctypes.c_void_p(stream or None)))

    def chess_ext_leaf_moves(self, first_game: int, n: int, flush: int, d_moves: int, d_depth: int, stream: int = 0):
        check(_CHESS.ext_leaf_moves(self._h, first_game, n, int(flush), ctypes.c_void_p(d_moves),
                                    ctypes.c_void_p(d_depth), ctypes.c_void_p(stream or None)))

    def debug_c4_puct_tree(self, game: int, max_nodes: int = 1 << 16) -> np.ndarray:
        """Game `game`'s Connect4 PUCT tree (test hook): node records (C4_PNODE_DTYPE)."""
        out = np.zeros(max_nodes, C4_PNODE_DTYPE)
        cnt = np.zeros(1, np.int32)
        check(lib().zc_debug_c4_puct_tree(self._h, int(game), max_nodes, _ptr(out), _ptr(cnt)))
        return out[:int(cnt[0])]

    def c4_rollouts(self, states: np.ndarray, game: int = 0):
        """Sequential rollouts of `states` on one game's stream: (values[n], words consumed)."""
        states = np.ascontiguousarray(states, dtype=C4_STATE_DTYPE)
        v = np.zeros(states.shape[0], np.int32)
        w = ctypes.c_int64(0)
        check(lib().zc_c4_rollouts(self._h, game, states.shape[0], _ptr(states), _ptr(v), ctypes.byref(w)))
        return v, w.value

    # ---- self-test hooks
    def debug_uct(self, logn, na, q, c: float):
        logn = np.ascontiguousarray(logn, np.float64)
        na = np.ascontiguousarray(na, np.int32)
        q = np.ascontiguousarray(q, np.float64)
        out = np.zeros(len(logn), np.float64)
        check(lib().zc_debug_uct(self._h, len(logn), _ptr(logn), _ptr(na), _ptr(q), float(c), _ptr(out)))
        return out

    def debug_c4_uct_select(self, child, na, wa, big_n, c: float):
        """The rollout search's UCT choice at node records child/na/wa [n, 8], big_n [n]:
        (slot [n], how [n]); how = 0 one fp32 candidate, 1 a tie of equal pairs, 2 fp64 fallback."""
        child = np.ascontiguousarray(child, np.uint16).reshape(-1, 8)
        na = np.ascontiguousarray(na, np.int32).reshape(-1, 8)
        wa = np.ascontiguousarray(wa, np.int32).reshape(-1, 8)
        big_n = np.ascontiguousarray(big_n, np.int32).reshape(-1)
        n = len(big_n)
        if not (len(child) == len(na) == len(wa) == n):
            raise ValueError("child, na, wa must be [n, 8] for big_n [n]")
        slot = np.zeros(n, np.int32)
        how = np.zeros(n, np.int32)
        check(lib().zc_debug_c4_uct_select(self._h, n, _ptr(child), _ptr(na), _ptr(wa), _ptr(big_n), float(c),
                                           _ptr(slot), _ptr(how)))
        return slot, how

    def phase_cycles_games(self, n: int) -> np.ndarray:
        """Per-game stamp cycles [n, 8] accumulated since the last phase_cycles() reset."""
        out = np.zeros((n, 8), np.int64)
        check(lib().zc_debug_phase_cycles_games(self._h, int(n), out.ctypes.data_as(P(ctypes.c_int64))))
        return out

    def phase_cycles(self, enable: bool):
        out = (ctypes.c_int64 * 8)()
        check(lib().zc_debug_phase_cycles(self._h, int(bool(enable)), out))
        return dict(zip(["rng", "walk_first", "walk_resumed", "expand", "rollout", "backup", "publish", "sub"],
                        list(out)))

    def debug_c4_rollout(self, states: np.ndarray, first_game: int = 0):
        states = np.ascontiguousarray(states, dtype=C4_STATE_DTYPE)
        n = states.shape[0]
        v = np.zeros(n, np.int32)
        w = np.zeros(n, np.int64)
        check(lib().zc_debug_c4_rollout(self._h, first_game, n, _ptr(states), _ptr(v), _ptr(w)))
        return v, w


def net_switch(name: str, value: int) -> int:
    """Set one of the network launches' switches (zc_debug_net_switch: "tower_mf", the MFMA form,
    0, 16 or 32; "head_raw", 0 or 1, for both widths); returns the previous value.  Any other
    name or value is refused."""
    old = ctypes.c_int32(0)
    check(lib().zc_debug_net_switch(name.encode(), int(value), ctypes.byref(old)))
    return old.value
