"""Host side of the fused encoder's frames beyond 256^2: the shape rule as one pure function, and the identity the kernels rest on --
for H a multiple of 32 and input_dim a multiple of 32 that divides H or is a multiple of it, AdaptiveAvgPool2d(input_dim) followed by
adaptive_avg_pool2d(32) is one (H/32)^2 block mean.  No GPU."""
import pytest
import torch
import torch.nn.functional as F


def test_hip_encoder_supported_states_the_rule():
    from smokephysai_amd.models.encoder import hip_encoder_supported
    for H in (64, 128, 256, 512, 1024):
        for input_dim in (32, 128, 256):
            assert hip_encoder_supported(H, H, input_dim), (H, input_dim)
    assert not hip_encoder_supported(96, 96, 128)
    assert not hip_encoder_supported(512, 256, 128)
    assert not hip_encoder_supported(256, 512, 128)
    assert not hip_encoder_supported(2048, 2048, 128)
    for H in (64, 256, 512, 1024):
        assert not hip_encoder_supported(H, H, 48), H
    assert not hip_encoder_supported(512, 512, 0)
    assert not hip_encoder_supported(512, 512, 96)            # a multiple of 32, neither a divisor nor a multiple of 512


def test_model_route_uses_the_same_rule():
    """SmokePhysNet._encoder_route asks hip_encoder_supported, not a list of its own."""
    import inspect

    from smokephysai_amd.models import smokephys_net
    src = inspect.getsource(smokephys_net.SmokePhysNet._encoder_route)
    assert "hip_encoder_supported(" in src and "(64, 128, 256)" not in src


@pytest.mark.parametrize("H", [512, 1024])
@pytest.mark.parametrize("input_dim", [32, 128, 256, 1024])
def test_two_adaptive_pools_compose_to_a_block_mean(H, input_dim):
    torch.manual_seed(H + input_dim)
    a = torch.rand(1, 4, H, H, dtype=torch.float64)
    two = F.adaptive_avg_pool2d(F.adaptive_avg_pool2d(a, input_dim), 32)
    P = H // 32
    block = a.reshape(1, 4, 32, P, 32, P).mean(dim=(3, 5))
    assert (two - block).abs().max().item() < 1e-12
