"""What the evaluation-cache flush entry points, zc_evalcache_clear_async and the tower entry points
refuse (include/zeroclone.h), pinned as a table that needs no GPU: every case changes one argument
of a valid call so that one check of the library fails, and the call must come back with
ZC_EINVAL — before any launch, so the pointers are made-up addresses of the right alignment that
nothing ever reads.  The valid argument sets themselves are called on the probes alone, with
n_rows = 0, where the library returns ZC_OK without a launch.
"""
import pytest

from zeroclone_amd import _native

EINVAL = _native.ZC_EINVAL


def _addr(i: int) -> int:
    return 0x100000 * (i + 1)   # distinct, aligned far beyond 16 bytes, never dereferenced


# name -> (argument names in the C order, {argument: valid value}); pointers start with "d_"
def _entry(names: str, **values):
    names = names.split()
    args = {n: _addr(i) if n.startswith("d_") else 0 for i, n in enumerate(names)}
    args.update(values)
    return names, args


_SIZES = dict(entries=64, key_bytes=24, logit_bytes=14)
_ROWS = dict(n_rows=4, rows_per_game=2, game_rows=3)

ENTRIES = {
    "zc_evalcache_clear_async": _entry("d_table entries key_bytes logit_bytes stream", **_SIZES),
    "zc_evalcache_probe_async": _entry(
        "d_table entries key_bytes logit_bytes n_rows rows_per_game game_rows d_keys d_planes plane_bytes "
        "d_out_values d_out_logits d_dense_planes d_miss_rows d_count d_stats stream",
        plane_bytes=6, **_SIZES, **_ROWS),
    "zc_evalcache_commit_async": _entry(
        "d_table entries key_bytes logit_bytes n_rows rows_per_game game_rows d_keys d_miss_rows d_count "
        "d_dense_values d_dense_logits d_out_values d_out_logits d_stats stream", **_SIZES, **_ROWS),
    "zc_evalcache_probe_merged_async": _entry(
        "d_table entries key_bytes logit_bytes n_rows rows_per_game game_rows d_keys d_planes plane_bytes "
        "d_out_values d_out_logits d_dense_planes d_miss_rows d_count d_stats d_scratch stream",
        plane_bytes=6, **_SIZES, **_ROWS),
    "zc_evalcache_commit_merged_async": _entry(
        "d_table entries key_bytes logit_bytes n_rows rows_per_game game_rows d_keys d_miss_rows d_count "
        "d_dense_values d_dense_logits d_out_values d_out_logits d_stats d_scratch stream", **_SIZES, **_ROWS),
    "zc_evalcache_probe_routed_async": _entry(
        "d_table_a d_table_b entries key_bytes logit_bytes n_rows rows_per_game game_rows d_route d_keys d_planes "
        "plane_bytes d_out_values d_out_logits d_dense_planes_a d_dense_planes_b d_miss_rows d_count d_stats "
        "d_scratch stream", plane_bytes=6, **_SIZES, **_ROWS),
    "zc_evalcache_commit_routed_async": _entry(
        "d_table_a d_table_b entries key_bytes logit_bytes n_rows rows_per_game game_rows d_keys d_miss_rows "
        "d_count d_dense_values_a d_dense_logits_a d_dense_values_b d_dense_logits_b d_out_values d_out_logits "
        "d_stats d_scratch stream", **_SIZES, **_ROWS),
    "zc_net_tower_async": _entry(
        "n h w cin0 nconv d_in d_packed d_bias d_out d_fc_w fc_b d_values stream",
        n=2, h=8, w=8, cin0=32, nconv=5, fc_b=0.0),
    "zc_net_tower_policy_async": _entry(
        "n h w cin0 nconv d_in d_packed d_bias d_fc_w fc_b d_values d_pw d_pb d_pout stream",
        n=2, h=8, w=8, cin0=32, nconv=5, fc_b=0.0),
    "zc_net_tower_policy_ex_async": _entry(
        "n h w cin0 nconv d_in d_packed d_bias d_fc_w fc_b d_values d_pw d_pb policy_channels relu d_pout stream",
        n=2, h=8, w=8, cin0=32, nconv=5, fc_b=0.0, policy_channels=32, relu=1),
    "zc_net_tower_counted_async": _entry(
        "n h w cin0 nconv d_in d_packed d_bias d_out d_fc_w fc_b d_values d_count stream",
        n=2, h=8, w=8, cin0=32, nconv=5, fc_b=0.0),
    "zc_net_tower_policy_counted_async": _entry(
        "n h w cin0 nconv d_in d_packed d_bias d_fc_w fc_b d_values d_pw d_pb policy_channels relu d_pout d_count "
        "stream", n=2, h=8, w=8, cin0=32, nconv=5, fc_b=0.0, policy_channels=32, relu=1),
}

CASES = []   # (entry point, case name, {argument: value})


def _case(fn: str, what: str, **changed):
    assert set(changed) <= set(ENTRIES[fn][1]), (fn, what)
    CASES.append((fn, what, changed))


def _null(fn: str, *pointers: str):
    for p in pointers:
        _case(fn, f"{p} null", **{p: 0})


def _misaligned(fn: str, mask: int, *pointers: str):
    """Each pointer off by every power of two within the mask the library tests."""
    for p in pointers:
        for bit in (1, 2, 4, 8):
            if bit & mask:
                _case(fn, f"{p} +{bit}", **{p: ENTRIES[fn][1][p] + bit})


def _sizes(fn: str):
    _case(fn, "key_bytes 0", key_bytes=0)
    _case(fn, "key_bytes 20", key_bytes=20)
    _case(fn, "key_bytes 520", key_bytes=520)
    _case(fn, "logit_bytes odd", logit_bytes=13)
    _case(fn, "logit_bytes negative", logit_bytes=-2)
    _case(fn, "entries negative", entries=-8)
    _case(fn, "entries past 2^30", entries=(1 << 30) + 1)


def _rows(fn: str):
    _case(fn, "n_rows negative", n_rows=-2)
    _case(fn, "rows_per_game 0", rows_per_game=0)
    _case(fn, "game_rows < rows_per_game", game_rows=1)
    _case(fn, "n_rows no multiple of rows_per_game", n_rows=3)
    _case(fn, "buffer rows 2^31", n_rows=1 << 16, rows_per_game=1, game_rows=1 << 15)
    _null(fn, "d_count")
    _misaligned(fn, 3, "d_count")
    _misaligned(fn, 7, "d_stats")


def _flush(fn: str):
    """The checks of a probe's or a commit's own pointers, by the argument names it has."""
    args = ENTRIES[fn][1]
    _sizes(fn)
    _rows(fn)
    if "plane_bytes" in args:
        _case(fn, "plane_bytes 0", plane_bytes=0)
        _case(fn, "plane_bytes odd", plane_bytes=7)
    for mask, names in ((7, "d_keys d_out_values d_dense_values d_dense_values_a d_dense_values_b"),
                        (3, "d_miss_rows d_route"),
                        (1, "d_planes d_out_logits d_dense_planes d_dense_planes_a d_dense_planes_b d_dense_logits "
                            "d_dense_logits_a d_dense_logits_b")):
        here = [n for n in names.split() if n in args]
        _null(fn, *here)
        _misaligned(fn, mask, *here)


# the table of the plain calls and of zc_evalcache_clear_async: there must be one
for _fn in ("zc_evalcache_clear_async", "zc_evalcache_probe_async", "zc_evalcache_commit_async"):
    _null(_fn, "d_table")
    _misaligned(_fn, 15, "d_table")
    _case(_fn, "entries 0 with a table", entries=0)
_sizes("zc_evalcache_clear_async")

# the merged calls: a table with its entries, or neither; the scratch is required
for _fn in ("zc_evalcache_probe_merged_async", "zc_evalcache_commit_merged_async"):
    _case(_fn, "entries 0 with a table", entries=0)
    _case(_fn, "entries without a table", d_table=0)
    _misaligned(_fn, 15, "d_table")
    _null(_fn, "d_scratch")
    _misaligned(_fn, 3, "d_scratch")

# the routed calls: two different tables with their entries, or none; the scratch is optional
for _fn in ("zc_evalcache_probe_routed_async", "zc_evalcache_commit_routed_async"):
    _case(_fn, "entries 0 with tables", entries=0)
    _case(_fn, "entries without tables", d_table_a=0, d_table_b=0)
    _case(_fn, "table A alone", d_table_b=0)
    _case(_fn, "table B alone", d_table_a=0)
    _case(_fn, "the two tables equal", d_table_b=ENTRIES[_fn][1]["d_table_a"])
    _misaligned(_fn, 15, "d_table_a", "d_table_b")
    _misaligned(_fn, 3, "d_scratch")
_case("zc_evalcache_probe_routed_async", "the two dense planes equal",
      d_dense_planes_b=ENTRIES["zc_evalcache_probe_routed_async"][1]["d_dense_planes_a"])

for _fn in ENTRIES:
    if "probe" in _fn or "commit" in _fn:
        _flush(_fn)

# the towers
for _fn in ENTRIES:
    if not _fn.startswith("zc_net_tower"):
        continue
    _case(_fn, "n negative", n=-1)
    _null(_fn, "d_in", "d_packed", "d_bias")
    _misaligned(_fn, 15, "d_in", "d_packed", "d_bias")
    if "policy" in _fn:
        _null(_fn, "d_fc_w", "d_values", "d_pw", "d_pb", "d_pout")
        _misaligned(_fn, 15, "d_pw")
        _misaligned(_fn, 7, "d_pout")
        if "policy_channels" in ENTRIES[_fn][1]:
            _misaligned(_fn, 15, "d_pb")
            _case(_fn, "policy_channels 48", policy_channels=48)
    else:
        _case(_fn, "neither d_out nor d_values", d_out=0, d_values=0)
        _case(_fn, "d_values without d_fc_w", d_fc_w=0)
        _misaligned(_fn, 15, "d_out")
    if "counted" in _fn:
        _null(_fn, "d_count")
        _misaligned(_fn, 3, "d_count")


def _call(fn: str, **changed) -> int:
    names, args = ENTRIES[fn]
    return getattr(_native.lib(), fn)(*({**args, **changed}[n] for n in names))


@pytest.mark.parametrize("fn,what,changed", CASES, ids=[f"{fn}-{what}".replace(" ", "_") for fn, what, _ in CASES])
def test_refused(fn, what, changed):
    assert _call(fn, **changed) == EINVAL


def test_every_case_is_its_own():
    assert len({(fn, what) for fn, what, _ in CASES}) == len(CASES)
    assert {fn for fn, _, _ in CASES} == set(ENTRIES)


PROBES = [fn for fn in ENTRIES if "probe" in fn]


@pytest.mark.parametrize("fn", PROBES)
def test_probe_of_no_rows_is_ok(fn):
    """The valid argument set, with n_rows 0: ZC_OK and no launch."""
    assert _call(fn, n_rows=0) == _native.ZC_OK


@pytest.mark.parametrize("fn", [fn for fn in PROBES if fn != "zc_evalcache_probe_async"])
def test_probe_of_no_rows_without_a_table_is_ok(fn):
    none = {n: 0 for n in ENTRIES[fn][1] if n.startswith("d_table")}
    assert _call(fn, n_rows=0, entries=0, **none) == _native.ZC_OK


def test_routed_probe_of_no_rows_without_a_scratch_is_ok():
    assert _call("zc_evalcache_probe_routed_async", n_rows=0, d_scratch=0) == _native.ZC_OK
