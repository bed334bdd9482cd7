"""CPU-side checks of the C-ABI library: it builds, loads, exports every declared symbol, and
its host-only helpers agree with the reference's fixtures.  No GPU compute here."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "zeroclone.h")


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"\b(zc_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def L():
    from zeroclone_amd import _native
    return _native.lib()


def test_every_declared_symbol_is_exported(L):
    from zeroclone_amd import _native
    syms = declared_symbols()
    assert len(syms) >= 15
    bound = {name for name, _, _ in _native.SIGNATURES}
    for s in syms:
        assert hasattr(L, s), s
        assert s in bound, f"{s} declared in zeroclone.h but not bound in _native.SIGNATURES"


def _kinds():
    import ctypes
    return {"int": ctypes.c_int, "i32": ctypes.c_int32, "i64": ctypes.c_int64, "u64": ctypes.c_uint64,
            "f64": ctypes.c_double, "f32": ctypes.c_float, "str": ctypes.c_char_p, "ptr": ctypes.c_void_p}


# (restype, argtypes) copied by hand from the binding's last hand-written table, typed pointers
# as "ptr": the whole type vocabulary and the longest argument lists
PINNED = {
    "zc_version": ("str", ""),
    "zc_last_error": ("str", ""),
    "zc_engine_create": ("int", "ptr ptr"),
    "zc_rng_seed": ("int", "ptr i32 i32 ptr"),
    "zc_c4_selfplay_pooled_async": ("int", "ptr i32 i32 ptr i32 f64 i32 i32 i64 ptr ptr ptr ptr ptr ptr"),
    "zc_chess_puct_begin_reuse": ("int", "ptr i32 i32 ptr i32 f64 i32 f32 f32 u64 ptr ptr ptr"),
    "zc_net_tower_policy_counted_w_async": ("int", "i32 i32 i32 i32 i32 i32 ptr ptr ptr ptr f32 ptr ptr ptr i32 i32 "
                                                   "ptr ptr ptr"),
    "zc_evalcache_probe_routed_async": ("int", "ptr ptr i64 i32 i32 i32 i32 i32 ptr ptr ptr i64 ptr ptr ptr ptr ptr "
                                               "ptr ptr ptr ptr"),
    "zc_train_loss_async": ("int", "i32 i32 i32 ptr i32 ptr ptr ptr ptr ptr ptr i64 ptr ptr ptr ptr"),
    "zc_chess_from_fen": ("int", "str ptr"),
}


def test_parsed_signatures_equal_the_pinned_sample():
    """The parser against declarations typed by hand: position by position, so a swapped pair
    of scalars or an int64 read as int32 shows."""
    from zeroclone_amd import _native
    kinds = _kinds()
    parsed = {name: (res, args) for name, res, args in _native.SIGNATURES}
    for name, (res, args) in PINNED.items():
        assert parsed[name][0] is kinds[res], name
        assert parsed[name][1] == [kinds[k] for k in args.split()], name


def test_every_declaration_is_parsed_once():
    from zeroclone_amd import _native
    names = [name for name, _, _ in _native.SIGNATURES]
    assert sorted(names) == declared_symbols()


def test_the_parser_maps_the_vocabulary_and_nothing_else():
    import ctypes
    from zeroclone_amd._native import parse_header
    sigs, _ = parse_header("/* c */ const char *zc_a(void);\n"
                           "int zc_b(zc_engine *eng, int64_t n,\n    const uint32_t *p, double, const char *s);\n"
                           "int zc_c(struct zc_unknown **, uint64_t seed, float t, uint32_t w, int32_t i);\n")
    assert sigs == [("zc_a", ctypes.c_char_p, []),
                    ("zc_b", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double,
                                            ctypes.c_char_p]),
                    ("zc_c", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_float, ctypes.c_uint32,
                                            ctypes.c_int32])]


@pytest.mark.parametrize("decl", [
    "int zc_bad(zc_engine *eng, size_t n);",                 # an unknown scalar type
    "int zc_bad(zc_engine *eng, unsigned int n);",
    "int zc_bad(zc_engine *eng, zc_c4_state root);",         # a struct by value
    "int zc_bad(zc_engine *eng, int32_t cols[7]);",          # an array parameter
    "int zc_bad(zc_engine *eng, void (*done)(int32_t));",    # a function pointer parameter
    "void zc_bad(zc_engine *eng);",                          # a return type outside the vocabulary
    "int zc_bad(zc_engine *eng, int32_t n) { return 0; }",   # a definition
    "int zc_bad(zc_engine *eng, int32_t);\nint zc_worse(",    # cut short
])
def test_the_parser_refuses_what_it_does_not_understand(decl):
    """No default to a pointer and no skipped line: the error names the declaration."""
    from zeroclone_amd._native import parse_header
    with pytest.raises(ValueError, match="zc_bad|zc_worse"):
        parse_header("int zc_good(int32_t n);\n" + decl + "\n")


def header_constants():
    text = open(HEADER).read()
    return {m[1]: m[2] for m in re.finditer(r"^#define (ZC_\w+)(.*)$", text, re.M)}


def test_constants_are_the_headers():
    from zeroclone_amd import _native
    defined = header_constants()
    assert len(defined) >= 43
    for name, rest in defined.items():   # every #define ZC_* is an integer and is published
        assert getattr(_native, name) == int(rest.split()[0]), name
    for name in dir(_native):   # and no ZC_* integer of the module disagrees with the header
        if name.startswith("ZC_") and name != "ZC_TRAJ_PI_MAX_COUNT":
            assert name in defined, f"{name} is not in zeroclone.h"


def test_legacy_aliases_are_the_headers_values():
    from zeroclone_amd import _native as n
    assert (n.ROLLOUT_EXACT, n.ROLLOUT_PHILOX) == (n.ZC_ROLLOUT_EXACT, n.ZC_ROLLOUT_PHILOX) == (0, 1)
    assert n.CHESS_MAX_MOVES == n.ZC_CHESS_MAX_MOVES == 256
    assert n.CHESS_ROLL_CAP == n.ZC_CHESS_ROLL_CAP == 2048
    assert n.ARENA_ROUTE_THREADS == n.ZC_ARENA_ROUTE_THREADS == 1024
    assert n.EVALCACHE_WAYS == n.ZC_EVALCACHE_WAYS == 8
    assert n.EVALCACHE_STATS == ("probed", "hits", "inserts", "dropped")
    assert n.EVALCACHE_MERGED_STATS == n.EVALCACHE_STATS + ("merged",)
    for i, name in enumerate(n.EVALCACHE_MERGED_STATS):
        assert getattr(n, "ZC_EVALCACHE_STAT_" + name.upper()) == i
    assert n.ZC_TRAJ_PI_MAX_COUNT == 65535


def test_version(L):
    assert b"gfx950" in L.zc_version()


def test_legal_order_table_matches_cpython(golden):
    from zeroclone_amd import _native
    order = golden("c4_set_order.json")["order"]
    for mask in range(128):
        assert _native.c4_legal_order(mask) == order[str(mask)]
        live = [m[0] for m in list({(i, 0) for i in range(7) if (mask >> i) & 1})]
        assert _native.c4_legal_order(mask) == live


def test_rows_roundtrip(golden):
    from zeroclone_amd import _native
    import ctypes
    for c in golden("c4_backend.json")["cases"][:100]:
        st = _native.c4_from_rows(c["board"], c["turn"])
        s = _native.C4State()
        s.stones[0] = int(st["stones"][0])
        s.stones[1] = int(st["stones"][1])
        s.turn = int(st["turn"])
        buf = ctypes.create_string_buffer(42)
        assert _native.lib().zc_c4_to_rows(ctypes.byref(s), buf) == 0
        back = buf.raw.decode().replace(" ", ".")
        assert back == c["board"]
        # bitboard legal mask == reference legal set
        occ = int(st["stones"][0]) | int(st["stones"][1])
        mask = sum(1 << col for col in range(7) if not (occ >> (7 * col + 5)) & 1)
        assert _native.c4_legal_order(mask) == c["legal"]


def test_invalid_arguments_fail_loudly(L):
    from zeroclone_amd import _native
    with pytest.raises(ValueError):
        _native.c4_from_rows("." * 42, 2)
    with pytest.raises(ValueError):
        _native.c4_legal_order(128)
