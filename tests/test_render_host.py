"""CPU tests of the volume render (SPEC_3D.md section 10): properties of the numpy oracle (tests/render_oracle.py) that pin the rule
itself -- identities, closed forms, the direction conventions -- the fp32 error budget the device tolerance is derived from, and the
host-side surface (header, binding, RenderSettings, render_supported, train.data_loader_kwargs).  No GPU.

fp32 budget: the float32 replay of the rule (segmented light prefix, z ascending) stays within 2e-6 max-norm relative of the float64 rule
over every shape, density, light and sigma pair of the device test (measured worst 7.9e-7, at (64, 128, 128)); the device bound, 1e-5, is ten times that
measurement: room for the device's exp and another summation order, a tenth of the project's 1e-4 bar."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import rel_err
from render_oracle import AMBIENT, DENSITIES, LIGHTS, SHAPES, SIGMAS, density, render_fp32_replay, render_fp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unlit_image_plus_transmittance_is_one():
    for kind in DENSITIES:
        for sv, _ in SIGMAS:
            img, T = render_fp64(density(kind, (24, 9, 11), seed=1), sv, 0.3, AMBIENT, 1.0, "none")
            assert np.abs(img + T - 1.0).max() <= 1e-12


def test_uniform_volume_is_a_geometric_series():
    D, rho, sv, sl, a, g = 12, 0.7, 0.3, 0.2, 0.25, 1.5
    vol = np.full((D, 5, 6), rho)
    q, alpha = np.exp(-sv * rho), -np.expm1(-sv * rho)
    img, T = render_fp64(vol, sv, sl, a, g, "none")
    np.testing.assert_allclose(img, g * alpha * (1 - q ** D) / (1 - q), rtol=1e-13)
    np.testing.assert_allclose(T, q ** D, rtol=1e-13)
    # "+z": the light crosses what the view ray crossed, A = tau = z rho: two geometric series
    img, _ = render_fp64(vol, sv, sl, a, g, "+z")
    q2 = np.exp(-(sv + sl) * rho)
    np.testing.assert_allclose(img, g * alpha * (a * (1 - q ** D) / (1 - q) + (1 - a) * (1 - q2 ** D) / (1 - q2)), rtol=1e-13)
    # "+y": A = y rho in row y, the same for every plane
    img, _ = render_fp64(vol, sv, sl, a, g, "+y")
    Ly = a + (1 - a) * np.exp(-sl * rho * np.arange(5))
    np.testing.assert_allclose(img, (g * alpha * (1 - q ** D) / (1 - q) * Ly)[:, None] * np.ones(6), rtol=1e-13)
    img2, _ = render_fp64(vol, sv, sl, a, g, "-y")
    np.testing.assert_allclose(img2, img[::-1], rtol=1e-13)


@pytest.mark.parametrize("light", LIGHTS)
def test_one_hot_volume_lights_one_pixel(light):
    D, H, W = 5, 7, 6
    for z, y, x in [(0, 0, 0), (D - 1, H - 1, W - 1), (2, 3, 4), (0, H - 1, 0), (D - 1, 0, W - 1)]:
        vol = np.zeros((D, H, W))
        vol[z, y, x] = 1.7
        img, T = render_fp64(vol, 0.4, 0.9, AMBIENT, 1.0, light)
        assert np.count_nonzero(img) == 1
        assert img[y, x] == -np.expm1(-0.4 * 1.7)                 # nothing in front of it, nothing between it and the light
        assert np.count_nonzero(T != 1.0) == 1 and T[y, x] == np.exp(-0.4 * 1.7)


def two_voxel_cases():
    """(name, light, voxel a, voxel b, which of them is dimmed: 'a', 'b' or None) on a (4, 6, 5) grid; both carry density 2."""
    return [("view: b behind a", "none", (0, 2, 2), (3, 2, 2), "b"),
            ("+y light: b below a in travel order", "+y", (1, 1, 3), (1, 4, 3), "b"),
            ("-y light: a is reached after b", "-y", (1, 1, 3), (1, 4, 3), "a"),
            ("+y light: other column", "+y", (1, 1, 3), (1, 4, 2), None),
            ("+y light: other plane", "+y", (1, 1, 3), (2, 4, 3), None),
            ("+z light: b behind a", "+z", (0, 2, 2), (3, 2, 2), "b"),
            ("+z light: side by side", "+z", (1, 2, 2), (1, 2, 3), None)]


def check_two_voxels(render, name, light, pa, pb, dimmed, exact):
    """render(vol, light) -> image; checks the direction convention of one two-voxel case.  Shared with the device test."""
    sv, sl, a, rho = 0.4, 0.9, AMBIENT, 2.0
    vol = np.zeros((4, 6, 5), np.float32)
    vol[pa] = vol[pb] = rho
    img = np.asarray(render(vol, light), np.float64)
    alpha, Tfront = -np.expm1(-sv * rho), np.exp(-sv * rho)
    shadow = a + (1 - a) * np.exp(-sl * rho)
    same_pixel = pa[1:] == pb[1:]
    want = {}
    if same_pixel:                                    # a in front of b on one view ray
        lit_b = shadow if light == "+z" else 1.0      # "+z": the front voxel also stands between the light and the back one
        want[pa[1:]] = alpha + alpha * lit_b * Tfront
    else:
        want[pa[1:]] = alpha * (shadow if dimmed == "a" else 1.0)
        want[pb[1:]] = alpha * (shadow if dimmed == "b" else 1.0)
    assert np.count_nonzero(img) == len(want), name
    for (y, x), w in want.items():
        np.testing.assert_allclose(img[y, x], w, rtol=exact, err_msg=name)
    if same_pixel:                                    # ... and not the reverse: swapping the densities' order changes nothing here, so
        vol2 = np.zeros_like(vol)                     # check the asymmetry with unequal densities: the back voxel never dims the front
        vol2[pa], vol2[pb] = 0.5, 3.0
        i2 = np.asarray(render(vol2, light), np.float64)[pa[1:]]
        lit = (a + (1 - a) * np.exp(-sl * 0.5)) if light == "+z" else 1.0
        np.testing.assert_allclose(i2, -np.expm1(-sv * 0.5) + -np.expm1(-sv * 3.0) * lit * np.exp(-sv * 0.5), rtol=exact, err_msg=name)


@pytest.mark.parametrize("case", two_voxel_cases(), ids=lambda c: c[0])
def test_two_voxel_directions(case):
    check_two_voxels(lambda vol, light: render_fp64(vol, 0.4, 0.9, AMBIENT, 1.0, light)[0], *case, exact=1e-14)


def test_plus_z_light_is_self_shadowing_along_the_view():
    rho = density("dense", (9, 6, 7), seed=2).astype(np.float64)
    sv, sl, a = 0.3, 0.7, AMBIENT
    img, _ = render_fp64(rho, sv, sl, a, 1.0, "+z")
    tau = np.cumsum(rho, 0) - rho
    want = np.sum(-np.expm1(-sv * rho) * (a * np.exp(-sv * tau) + (1 - a) * np.exp(-(sv + sl) * tau)), 0)
    np.testing.assert_allclose(img, want, rtol=1e-13)


@pytest.mark.parametrize("light", LIGHTS)
def test_bounds(light):
    for kind in DENSITIES:
        for sv, sl in SIGMAS:
            img, T = render_fp64(density(kind, (16, 20, 12), seed=3), sv, sl, AMBIENT, 1.0, light)
            assert img.min() >= 0.0 and np.all(img <= (1.0 - T) * (1 + 1e-12))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_fp32_replay_stays_within_2e_6_of_fp64(shape):
    worst = 0.0
    for kind in DENSITIES:
        rho = density(kind, shape)
        for sv, sl in SIGMAS:
            for light in LIGHTS:
                want, wantT = render_fp64(rho, sv, sl, AMBIENT, 1.0, light)
                got, gotT = render_fp32_replay(rho, sv, sl, AMBIENT, 1.0, light)
                e = rel_err(got, want)
                worst = max(worst, e)
                assert e <= 2e-6, (shape, kind, sv, sl, light, e)
                assert np.abs(gotT - wantT).max() <= 2e-6, (shape, kind, sv, sl, light)
    print(f"fp32 replay vs fp64 at {shape}: worst {worst:.2e}")


def test_alpha_needs_expm1():
    """alpha = 1 - exp(-x) loses the small arguments: several times the error of expm1 in the same fp32 replay."""
    rho = density("sparse", (24, 70, 64))
    want, _ = render_fp64(rho, 0.02, 0.05, AMBIENT, 1.0, "none")
    good = rel_err(render_fp32_replay(rho, 0.02, 0.05, AMBIENT, 1.0, "none")[0], want)
    bad = rel_err(render_fp32_replay(rho, 0.02, 0.05, AMBIENT, 1.0, "none", expm1=False)[0], want)
    print(f"alpha by expm1 {good:.2e}, by 1 - exp {bad:.2e}")
    assert good <= 2e-6 and bad > 2 * good


def test_shapes_span_three_row_segments_with_a_remainder():
    from smokephysai_amd.physics import render
    seg = render.SEGMENT_ROWS
    if not seg:
        pytest.skip("the mapping has no row segments")
    assert any(H // seg >= 3 and H % seg for _, H, _ in SHAPES), seg
    assert any(H < seg for _, H, _ in SHAPES) and any(H % seg == 0 and H // seg > 1 for _, H, _ in SHAPES)
    src = open(os.path.join(ROOT, "smokephysai_amd", "csrc", "render.h")).read()
    assert int(re.search(r"RENDER_SEG_ROWS\s*=\s*(\d+)", src).group(1)) == seg
    assert int(re.search(r"RENDER_MAX_DEPTH\s*=\s*(\d+)", src).group(1)) == render.MAX_DEPTH == 64


def test_header_binding_and_abi_version():
    from smokephysai_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION      # additive: the version stays
    assert re.search(r"int64_t\s+smk_volume_render_workspace\(", hdr) and re.search(r"int\s+smk_volume_render\(", hdr)
    assert "smk_render_desc" in hdr and "smk_light" in hdr
    for name in ("smk_volume_render", "smk_volume_render_workspace"):
        assert name in _lib.EXPORTS
    L = _lib.load()
    assert L.smk_abi_version() == 17
    for name in ("smk_volume_render", "smk_volume_render_workspace"):
        assert hasattr(L, name)
    # the enum of the header and the binding's constants
    enum = dict(re.findall(r"(SMK_LIGHT_\w+)\s*=\s*(\d+)", hdr))
    assert {k: int(v) for k, v in enum.items()} == {k: getattr(_lib, k) for k in ("SMK_LIGHT_NONE", "SMK_LIGHT_POS_Y", "SMK_LIGHT_NEG_Y", "SMK_LIGHT_POS_Z")}
    # the workspace rule needs no device: none for the unlit / +z lights and for one segment, [n][segments][D][W] floats otherwise
    assert L.smk_volume_render_workspace(3, 24, 70, 64, _lib.SMK_LIGHT_NONE) == 0
    assert L.smk_volume_render_workspace(3, 24, 70, 64, _lib.SMK_LIGHT_POS_Z) == 0
    assert L.smk_volume_render_workspace(3, 24, 16, 64, _lib.SMK_LIGHT_POS_Y) == 0
    assert L.smk_volume_render_workspace(3, 24, 70, 64, _lib.SMK_LIGHT_NEG_Y) == 3 * 5 * 24 * 64 * 4
    assert L.smk_volume_render_workspace(1, 65, 8, 8, _lib.SMK_LIGHT_NONE) == -1
    assert L.smk_volume_render_workspace(1, 64, 8, 8, 4) == -1
    assert L.smk_volume_render_workspace(1, 64, 8192, 8192, _lib.SMK_LIGHT_NONE) == -1


def test_render_settings_refuse_bad_values():
    from smokephysai_amd.physics import RenderSettings
    s = RenderSettings()
    assert (s.sigma_view, s.sigma_light, s.ambient, s.gain, s.light) == (0.1, 0.1, 0.25, 1.0, "-y")
    with pytest.raises(Exception):
        s.gain = 2.0                                   # frozen
    RenderSettings(0.0, 0.0, 0.0, 1e-3, "none"), RenderSettings(4, 8, 1, 2, "+z")
    for bad in (dict(sigma_view=-0.1), dict(sigma_view=float("nan")), dict(sigma_light=float("inf")), dict(sigma_light=-1),
                dict(ambient=-0.01), dict(ambient=1.01), dict(ambient=float("nan")), dict(gain=0.0), dict(gain=-1.0),
                dict(gain=float("inf")), dict(light="y"), dict(light="+x"), dict(light=None), dict(sigma_view="0.1")):
        with pytest.raises(ValueError):
            RenderSettings(**bad)


def test_render_supported():
    from smokephysai_amd.physics import render_supported
    assert render_supported(1, 1, 1) and render_supported(64, 512, 512) and render_supported(16, 300, 40)
    assert not render_supported(65, 8, 8) and not render_supported(0, 8, 8) and not render_supported(8, 0, 8) and not render_supported(8, 8, 0)
    assert render_supported(64, 4096, 8191) and not render_supported(64, 8192, 4096)       # 2^31 - 2^16 cells at most
    with pytest.raises(TypeError):
        render_supported(8.0, 8, 8)


def test_render_volumes_refuses_without_a_device():
    import torch
    from smokephysai_amd.physics import render_volumes
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_volumes(torch.zeros(2, 4, 4))


def _config(hw=None):
    cfg = {"training": {"batch_size": 4}, "data": {"num_train": 6, "num_val": 2, "grid_size": [64, 64], "cache_dir": None}}
    if hw is not None:
        cfg["mi355x"] = hw
    return cfg


def test_data_loader_kwargs_forward_render_depth_only_when_set():
    import yaml
    import train
    from smokephysai_amd.utils import data_loader
    base = dict(batch_size=4, num_train=6, num_val=2, grid_size=(64, 64), cache_dir=None, sim_batch=64, jacobi_iters=20, labels="host",
                rank=0, world=1)
    assert train.data_loader_kwargs(_config()) == base
    assert train.data_loader_kwargs(_config({"render_depth": 0, "render": {"light": "+y"}})) == base
    kw = train.data_loader_kwargs(_config({"render_depth": 16, "render": {"light": "+y", "sigma_view": 0.2}, "sim_batch": 4}))
    assert kw == dict(base, sim_batch=4, render_depth=16, render={"light": "+y", "sigma_view": 0.2})
    assert train.data_loader_kwargs(_config({"render_depth": 8}))["render"] == {}
    accepted = set(inspect.signature(data_loader.create_data_loaders).parameters) | set(
        inspect.signature(data_loader.SyntheticSmokeDataset3D.__init__).parameters) | {"labels"}
    assert set(kw) <= accepted
    # a bad setting fails in the dataset's own check, without a GPU
    with pytest.raises(ValueError, match="light"):
        data_loader.create_data_loaders(device="cuda", **train.data_loader_kwargs(_config({"render_depth": 16, "render": {"light": "up"}})))
    with pytest.raises(ValueError):
        data_loader.create_data_loaders(device="cuda", **train.data_loader_kwargs(_config({"render_depth": 65})))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "config.yaml")))
    assert cfg["mi355x"]["render_depth"] == 0
    assert cfg["mi355x"]["render"] == dict(sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y")
    assert "render_depth" not in train.data_loader_kwargs(cfg)
    assert data_loader.as_render_settings(cfg["mi355x"]["render"]) == data_loader.as_render_settings(None)
