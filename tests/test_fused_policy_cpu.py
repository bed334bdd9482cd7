"""CPU-side checks of the fused launches' visit-count recording: the switch's refusal, which
needs no device, and the new entry points' place in the header and the binding."""
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "zeroclone.h")
NEW_SYMBOLS = ("zc_c4_selfplay_visits", "zc_chess_selfplay_visits", "zc_traj_policy_steps_scratch_bytes",
               "zc_traj_policy_record_steps_async")


@pytest.mark.parametrize("pool", ["C4SelfPlay", "ChessSelfPlay"])
def test_fused_policy_needs_record_policy(pool, monkeypatch):
    """fused_policy without record_policy raises before any engine or device buffer is made."""
    from zeroclone_amd import _native, selfplay

    def no_device(*a, **k):
        raise AssertionError("the refusal must come before an engine is created")

    monkeypatch.setattr(_native, "NativeEngine", no_device)
    with pytest.raises(ValueError, match="record_policy"):
        getattr(selfplay, pool)(4, 32, fused_policy=True)


@pytest.mark.parametrize("pool", ["C4SelfPlay", "ChessSelfPlay"])
def test_the_older_refusals_come_first_and_unchanged(pool, monkeypatch):
    """With the switch on, a count that does not fit 16 bits is still refused, in the same words."""
    from zeroclone_amd import _native, selfplay
    monkeypatch.setattr(_native, "NativeEngine", lambda *a, **k: pytest.fail("no engine expected"))
    with pytest.raises(ValueError, match="65535"):
        getattr(selfplay, pool)(4, 65536, record_policy=True, fused_policy=True)


def test_new_entry_points_are_declared_exported_and_bound():
    from zeroclone_amd import _native
    text = open(HEADER).read()
    bound = {name: args for name, _, args in _native.SIGNATURES}
    for s in NEW_SYMBOLS:
        decl = re.search(r"^int %s\((.*?)\);" % s, text, re.S | re.M)
        assert decl, s
        assert hasattr(_native.lib(), s), s
        assert len(bound[s]) == decl.group(1).count(",") + 1, s


def test_record_steps_keeps_refusing_a_policy_pool_without_the_staging():
    """Trajectories.record_steps' refusal is raised before anything is enqueued; its text is
    the one callers of the fused launches have always seen."""
    from zeroclone_amd import selfplay
    t = object.__new__(selfplay.Trajectories)
    t.quota, t.policy_width = selfplay._UNLIMITED, 7
    with pytest.raises(ValueError, match="export no per-move visit counts"):
        t.record_steps(0, None, None, 4)
