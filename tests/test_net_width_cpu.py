"""The network widths the MFMA towers cover (64 and 128 channels): what needs no GPU."""
import pytest
import torch


def test_mfma_supported_widths():
    from zeroclone_amd.nets import ValueNetwork, mfma_supported
    assert mfma_supported(ValueNetwork(64, 1, 2))
    assert mfma_supported(ValueNetwork(128, 1, 17))
    for channels in (32, 96, 256):
        assert not mfma_supported(ValueNetwork(channels, 1, 2)), channels
    assert not mfma_supported(ValueNetwork(64, 1, 33))
    assert not mfma_supported(ValueNetwork(128, 1, 33))


@pytest.mark.parametrize("P", [32, 64])
def test_pack_policy_1x1_at_64_channels(P):
    """[P, 64] -> [P / 16 M tiles][2 k-steps][64 lanes][8]: lane l of k-step j of M tile mt holds
    weight[16 mt + l % 16, 32 j + 8 (l // 16) + e] — the A operand of v_mfma_f32_16x16x32_f16."""
    from zeroclone_amd.nets import pack_policy_1x1
    w = torch.arange(P * 64, dtype=torch.float32).reshape(P, 64)   # every element its own index
    got = pack_policy_1x1(w)
    assert got.shape == (P // 16, 2, 64, 8) and got.is_contiguous()
    want = torch.empty(P // 16, 2, 64, 8)
    for mt in range(P // 16):
        for j in range(2):
            for lane in range(64):
                for e in range(8):
                    want[mt, j, lane, e] = (16 * mt + lane % 16) * 64 + 32 * j + 8 * (lane // 16) + e
    assert torch.equal(got, want)


def test_pack_policy_1x1_at_128_channels_is_unchanged():
    """[P, 128] keeps the 32x32x16 layout: lane l of k-step kc of block mb holds
    weight[32 mb + l % 32, 16 kc + 8 (l // 32) + e]."""
    from zeroclone_amd.nets import pack_policy_1x1
    w = torch.arange(64 * 128, dtype=torch.float32).reshape(64, 128)
    got = pack_policy_1x1(w)
    assert got.shape == (2, 8, 64, 8)
    for mb, kc, lane, e in [(0, 0, 0, 0), (1, 7, 63, 7), (0, 3, 37, 2), (1, 0, 31, 5)]:
        assert got[mb, kc, lane, e].item() == (32 * mb + lane % 32) * 128 + 16 * kc + 8 * (lane // 32) + e


@pytest.mark.parametrize("shape", [(48, 64), (32, 96), (16, 64), (64, 32)])
def test_pack_policy_1x1_refuses_other_shapes(shape):
    from zeroclone_amd.nets import pack_policy_1x1
    with pytest.raises(ValueError, match="64 or 128"):
        pack_policy_1x1(torch.zeros(shape))


def test_inference_form_on_the_cpu_is_the_folded_module():
    from zeroclone_amd import learner, nets
    model = nets.ValueNetwork(64, 1, 2)
    form = learner.inference_form(model, "cpu")
    assert isinstance(form, nets.FoldedValueNetwork)
    pmodel = nets.PolicyValueNetwork(64, 1, in_planes=2, board=(6, 7), n_logits=7)
    assert isinstance(learner.inference_form(pmodel, "cpu"), learner.FoldedPolicyValueNetwork)


def test_refusals_name_both_widths():
    from zeroclone_amd.selfplay import _check_mfma
    with pytest.raises(ValueError, match="64 or 128 channels"):
        _check_mfma((torch.nn.Identity(),), ())
