"""The arena pools' eval_cache / eval_merge refusals: a network that is not the MFMA form cannot
take its row count from the device, and the arena says so before any engine exists (no GPU)."""
import pytest

from arena_nets import ExactModel
from zeroclone_amd.arena import C4Arena, ChessArena
from zeroclone_amd.nets import PolicyValueNetwork, ValueNetwork

SWITCHES = [dict(eval_cache=1 << 10), dict(eval_merge=True), dict(eval_cache=1 << 10, eval_merge=True)]


@pytest.mark.parametrize("kw", SWITCHES, ids=["cache", "merge", "both"])
def test_arena_cache_refuses_torch_modules(kw):
    with pytest.raises(ValueError, match="MFMA"):
        C4Arena(8, 64, net_a=ValueNetwork(128, 1, in_planes=2), net_b=ValueNetwork(128, 1, in_planes=2), **kw)
    with pytest.raises(ValueError, match="MFMA"):
        ChessArena(8, 64, puct_net_a=PolicyValueNetwork(blocks=1), puct_net_b=PolicyValueNetwork(blocks=1), **kw)


@pytest.mark.parametrize("kw", SWITCHES, ids=["cache", "merge", "both"])
def test_arena_cache_refuses_exact_models(kw):
    with pytest.raises(ValueError, match="MFMA"):
        C4Arena(8, 64, net_a=ExactModel(1), net_b=ExactModel(2), **kw)
    with pytest.raises(ValueError, match="MFMA"):
        ChessArena(8, 64, puct_net_a=ExactModel(1, 4096), puct_net_b=ExactModel(2, 4096), **kw)


def test_the_message_names_the_switches():
    for kw in SWITCHES:
        with pytest.raises(ValueError, match="eval_cache / eval_merge"):
            C4Arena(8, 64, net_a=object(), net_b=object(), **kw)
