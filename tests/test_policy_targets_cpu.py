"""CPU-side checks of the policy-target recorder's binding: the ctypes struct against the
header's, and the refusals that need no device."""
import ctypes
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "zeroclone.h")
C_TYPES = {"int32_t": (ctypes.c_int32, 4), "int64_t": (ctypes.c_int64, 8)}


def header_fields(struct: str):
    """(name, size, is_pointer) of each field of `struct`'s body in include/zeroclone.h, in order."""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s+(.*)", decl, re.S)
        ctype, names = m.group(1), [n.strip() for n in m.group(2).split(",")]
        for n in names:
            ptr = n.startswith("*")
            out.append((n.lstrip("*").strip(), 8 if ptr else C_TYPES[ctype][1], ptr))
    return out


def test_policy_struct_matches_the_header():
    from zeroclone_amd import _native
    want = header_fields("zc_traj_policy_buffers")
    got = _native.TrajPolicyBuffers._fields_
    assert [n for n, _, _ in want] == [n for n, _ in got]
    off = 0
    for (name, size, ptr), (_, ctype) in zip(want, got):
        assert ctypes.sizeof(ctype) == size, name
        assert (ctype is ctypes.c_void_p) == ptr, name
        off = (off + size - 1) // size * size   # natural alignment, as the C compiler lays it out
        assert getattr(_native.TrajPolicyBuffers, name).offset == off, name
        off += size
    assert ctypes.sizeof(_native.TrajPolicyBuffers) == (off + 7) // 8 * 8 == 72
    # the parser reads the existing struct the same way
    assert [n for n, _, _ in header_fields("zc_traj_buffers")] == [n for n, _ in _native.TrajBuffers._fields_]


def test_policy_constants_match_the_header():
    from zeroclone_amd import _native
    text = open(HEADER).read()
    for name in ("ZC_TRAJ_PI_ENTRIES", "ZC_TRAJ_PI_OVERFLOW"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(_native, name)
    assert _native.ZC_TRAJ_PI_MAX_COUNT == (1 << 16) - 1


@pytest.mark.parametrize("pool", ["C4SelfPlay", "ChessSelfPlay"])
def test_more_simulations_than_a_count_holds_are_refused(pool, monkeypatch):
    """record_policy stores 16-bit counts: sims > 65535 raises before any engine or device
    buffer is made."""
    from zeroclone_amd import _native, selfplay

    def no_device(*a, **k):
        raise AssertionError("the refusal must come before an engine is created")

    monkeypatch.setattr(_native, "NativeEngine", no_device)
    with pytest.raises(ValueError, match="65535"):
        getattr(selfplay, pool)(4, 65536, record_policy=True)


def test_policy_recording_needs_the_trajectories(monkeypatch):
    from zeroclone_amd import _native, selfplay
    monkeypatch.setattr(_native, "NativeEngine", lambda *a, **k: pytest.fail("no engine expected"))
    with pytest.raises(ValueError, match="record"):
        selfplay.C4SelfPlay(4, 32, record=False, record_policy=True)


def test_trajbatch_positional_construction_still_works():
    from zeroclone_amd.selfplay import TrajBatch
    b = TrajBatch(1, 2, 3, 4)
    assert (b.rows, b.labels, b.moves, b.games, b.pi_off, b.pi) == (1, 2, 3, 4, None, None)
