"""Attention maps, the parts that need no GPU: ChaosAttention.attention_maps' PyTorch route against the reference's unfolded formula
(chaos_attention.py:82-108) in fp64, the construction the GPU tests reuse to get maps that are far from uniform, the support predicate,
SmokeVisualizer's three figures and inference.py's --attention-maps flag."""
import os

import pytest
import torch

from attention_maps_cases import module_inputs, peaked_module, reference_probs
from smokephysai_amd.models.attention import hip_attention_maps_supported, hip_attention_supported


def test_torch_route_equals_the_reference_formula_in_fp64():
    m = peaked_module(weight_scale=1.0).double()
    x, noise = (t.double() for t in module_inputs())
    with torch.no_grad():
        ref = reference_probs(m, x, noise)
    received, probs = m.attention_maps(x, noise=noise, probs_for=(0, 2, 0, 2))
    assert probs.shape == (2, 2, 128, 128) and received.shape == (2, 2, 128) and probs.dtype == torch.float64
    assert float((probs - ref).abs().max()) < 1e-12
    assert torch.equal(received, probs.mean(2))
    assert float((received.sum(-1) - 1).abs().max()) < 1e-12
    assert torch.equal(m.attention_maps(x, noise=noise), received)                       # without probs_for: the map alone
    _, sub = m.attention_maps(x, noise=noise, probs_for=(1, 1, 1, 1))
    assert torch.equal(sub, probs[1:2, 1:2])
    assert not received.requires_grad and not probs.requires_grad                        # no_grad, parameters with requires_grad


def test_torch_route_applies_a_key_mask():
    m = peaked_module().double()
    x, noise = (t.double() for t in module_inputs())
    mask = torch.ones(2, 128)
    mask[:, 100:] = 0
    received, probs = m.attention_maps(x, noise=noise, probs_for=(0, 2, 0, 2), mask=mask)
    assert float(probs[..., 100:].abs().max()) == 0.0 and float(received[..., 100:].abs().max()) == 0.0
    assert float((probs.sum(-1) - 1).abs().max()) < 1e-12


def test_scaled_projections_give_maps_far_from_uniform():
    """The GPU module test must not compare two nearly uniform maps: with q_proj / k_proj scaled by 4 every (batch, head) has a key that
    receives more than twice the uniform share."""
    x, noise = (t.double() for t in module_inputs())
    peak = {}
    for scale in (1.0, 4.0):
        m = peaked_module(weight_scale=scale).double()
        received = m.attention_maps(x, noise=noise)
        peak[scale] = float((received.max(-1).values * 128).min())
    print(f"min over (b, h) of max_j received * L: {peak}")
    assert peak[4.0] > 2.0
    assert peak[1.0] < peak[4.0]


@pytest.mark.parametrize("L", (64, 128, 192, 1024))
@pytest.mark.parametrize("head_dim", (32, 64))
def test_maps_predicate(L, head_dim):
    want = head_dim == 64 and L in (128, 1024)
    assert hip_attention_maps_supported(L, head_dim) is want
    assert hip_attention_maps_supported(L, head_dim) == hip_attention_supported(L, head_dim)


# ------------------------------------------------------------------------------------------------ SmokeVisualizer
def _panels(fig):
    return [ax for ax in fig.axes if ax.get_label() != "<colorbar>"]


@pytest.fixture
def viz():
    import matplotlib.pyplot as plt
    from smokephysai_amd.utils import SmokeVisualizer
    yield SmokeVisualizer()
    plt.close("all")


def _nonempty_png(path):
    with open(path, "rb") as f:
        head = f.read(8)
    return head == b"\x89PNG\r\n\x1a\n" and os.path.getsize(path) > 1000


def test_visualizer_smoke_evolution(viz, tmp_path):
    g = torch.Generator().manual_seed(0)
    frames = [torch.rand(16, 16, generator=g) for _ in range(8)] + [torch.rand(16, 16, generator=g).numpy()]
    path = str(tmp_path / "evolution.png")
    fig = viz.plot_smoke_evolution(frames, save_path=path)
    assert _nonempty_png(path)
    assert len(fig.axes) == 16                                                # 9 frames: 2 rows of 8
    assert [ax.get_title() for ax in fig.axes[:9]] == [f"Frame {i}" for i in range(9)]
    assert sum(bool(ax.images) for ax in fig.axes) == 9


def test_visualizer_chaos_features_with_a_missing_metric(viz, tmp_path):
    path = str(tmp_path / "chaos.png")
    fig = viz.plot_chaos_features({"lyapunov_exponent": [0.1, 0.2, 0.15], "entropy": [1.0, 1.1, 1.3]}, save_path=path)
    assert _nonempty_png(path)
    assert [bool(ax.lines) for ax in fig.axes] == [True, False, True]
    assert [ax.get_title() for ax in fig.axes] == ["Lyapunov Exponent", "", "Entropy"]


def test_visualizer_attention_maps(viz, tmp_path):
    g = torch.Generator().manual_seed(0)
    image = torch.rand(2, 1, 8, 8, generator=g)
    square = torch.softmax(torch.randn(2, 2, 16, 16, generator=g), -1)
    odd = torch.softmax(torch.randn(2, 2, 12, 12, generator=g), -1)
    figs = {}
    for name, kw in (("square", dict(attention_weights=square)), ("odd", dict(attention_weights=odd)),
                     ("received", dict(attention_weights=None, received=square.mean(2).view(2, 2, 4, 4))),
                     ("both", dict(attention_weights=square, received=square.mean(2).view(2, 2, 4, 4)))):
        path = str(tmp_path / f"{name}.png")
        figs[name] = viz.plot_attention_maps(input_image=image, save_path=path, **kw)
        assert _nonempty_png(path), name
    titles = {name: [ax.get_title() for ax in _panels(fig)] for name, fig in figs.items()}
    assert titles["square"] == ["Input Smoke", "Attention Matrix", "Average Attention"]
    assert titles["odd"] == ["Input Smoke", "Attention Matrix"]               # L = 12 is no square: one panel fewer
    assert len(_panels(figs["odd"])) == len(_panels(figs["square"])) - 1
    assert titles["received"] == ["Input Smoke", "Average Attention"]
    assert titles["both"] == titles["square"]
    # the third panel of the weights-only form is weights[0, 0].mean(0) as sqrt(L) x sqrt(L) (visualization.py:102-106)
    drawn = _panels(figs["square"])[2].images[0].get_array()
    assert drawn.shape == (4, 4)
    assert float(abs(torch.as_tensor(drawn.data) - square[0, 0].mean(0).view(4, 4)).max()) < 1e-7
    with pytest.raises(ValueError):
        viz.plot_attention_maps(None, image)


def test_visualizer_is_exported_lazily():
    import smokephysai_amd.utils as utils
    assert "SmokeVisualizer" in utils.__all__
    from smokephysai_amd.utils.visualization import SmokeVisualizer
    assert utils.SmokeVisualizer is SmokeVisualizer


# ------------------------------------------------------------------------------------------------ inference.py
def test_inference_parser_attention_maps_flag():
    import inference
    parser = inference.build_parser()
    assert parser.parse_args(["--checkpoint", "x"]).attention_maps is None
    assert parser.parse_args(["--checkpoint", "x", "--attention-maps"]).attention_maps == -1      # the last layer
    assert parser.parse_args(["--checkpoint", "x", "--attention-maps", "3"]).attention_maps == 3


def test_model_attention_maps_refuses_train_mode():
    from smokephysai_amd.models import SmokePhysNet
    model = SmokePhysNet(hidden_dim=128, num_heads=2, num_layers=1)
    with pytest.raises(RuntimeError, match="eval mode"):
        model.attention_maps(torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError, match="layers"):
        model.eval().attention_maps(torch.zeros(1, 1, 64, 64), layers=[1])
