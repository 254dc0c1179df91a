"""GPU tests of the volume render (SPEC_3D.md section 10): smk_volume_render (csrc/render.hip) through render_volumes, SmokeSimulator3D's
render / simulate_frames, RenderedSmokeDataset and create_data_loaders(render_depth=...), against tests/render_oracle.py.

Bounds:
  image: 1e-5 max-norm relative (conftest.rel_err) against the float64 rule; transmittance: 1e-5 absolute.  The float32 replay of the rule
      on the CPU stays within 7.9e-7 of float64 over these very shapes and settings (tests/test_render_host.py); 1e-5 is ten times that,
      room for the device's exp and another summation order, and a tenth of the project's 1e-4 bar.  Measured on MI355X: image 7.4e-7 at worst
      (at (64, 128, 128)), transmittance 1.8e-7.
  one-hot and two-voxel cases: rtol 1e-6 of the closed form (a handful of fp32 operations).
  everything stated as "equal" is bit for bit (torch.equal)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import rel_err                                                                                       # noqa: E402
from render_oracle import AMBIENT, DENSITIES, LIGHTS, SHAPES, SIGMAS, density, render_fp64                         # noqa: E402
from smokephysai_amd import _lib                                                                                   # noqa: E402
from smokephysai_amd.physics import RenderSettings, SmokeSimulator3D, render_volumes, render_workspace             # noqa: E402
from smokephysai_amd.utils.data_loader import RenderedSmokeDataset, SyntheticSmokeDataset3D, create_data_loaders   # noqa: E402
from test_render_host import check_two_voxels, two_voxel_cases                                                     # noqa: E402

DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- a. against the fp64 oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_render_matches_the_fp64_rule(shape):
    worst_img, worst_T = 0.0, 0.0
    for kind in DENSITIES:
        rho = density(kind, shape)
        vol = _dev(rho)
        for sv, sl in SIGMAS:
            for light in LIGHTS:
                want, wantT = render_fp64(rho, sv, sl, AMBIENT, 1.0, light)
                img, T = render_volumes(vol, RenderSettings(sv, sl, AMBIENT, 1.0, light), transmittance=True)
                assert img.shape == T.shape == shape[1:]
                e, eT = rel_err(img.cpu().numpy(), want), float(np.abs(T.cpu().numpy() - wantT).max())
                worst_img, worst_T = max(worst_img, e), max(worst_T, eT)
                assert e <= 1e-5, (shape, kind, sv, sl, light, e)
                assert eT <= 1e-5, (shape, kind, sv, sl, light, eT)
    print(f"render {shape}: worst image rel err {worst_img:.2e}, worst transmittance abs err {worst_T:.2e}")


def test_gain_and_ambient_scale_as_the_rule_says():
    rho = density("dense", (5, 33, 36), seed=4)
    for a, g in [(0.0, 0.5), (1.0, 3.0), (0.6, 1.0)]:
        want, _ = render_fp64(rho, 0.3, 0.7, a, g, "+y")
        got = render_volumes(_dev(rho), RenderSettings(0.3, 0.7, a, g, "+y"))
        assert rel_err(got.cpu().numpy(), want) <= 1e-5, (a, g)


# ---- b. one-hot and direction cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", LIGHTS)
def test_one_hot_volume_lights_one_pixel(light):
    D, H, W = 5, 37, 70                                     # three row segments with a remainder, two column chunks of 64
    spots = [(0, 0, 0), (D - 1, H - 1, W - 1), (2, 17, 64), (0, H - 1, 0), (D - 1, 0, W - 1), (3, 16, 63)]
    vols = np.zeros((len(spots), D, H, W), np.float32)
    for i, p in enumerate(spots):
        vols[(i,) + p] = 1.7
    img, T = render_volumes(_dev(vols), RenderSettings(0.4, 0.9, AMBIENT, 1.0, light), transmittance=True)
    img, T = img.cpu().numpy(), T.cpu().numpy()
    for i, (z, y, x) in enumerate(spots):
        assert np.count_nonzero(img[i]) == 1, (light, spots[i])
        np.testing.assert_allclose(img[i, y, x], -np.expm1(-0.4 * 1.7), rtol=1e-6)
        assert np.count_nonzero(T[i] != 1.0) == 1
        np.testing.assert_allclose(T[i, y, x], np.exp(-0.4 * 1.7), rtol=1e-6)


@pytest.mark.parametrize("case", two_voxel_cases(), ids=lambda c: c[0])
def test_two_voxel_directions(case):
    check_two_voxels(lambda vol, light: render_volumes(_dev(vol), RenderSettings(0.4, 0.9, AMBIENT, 1.0, light)).cpu().numpy(), *case,
                     exact=1e-6)


def test_shadow_crosses_row_segments():
    """A voxel in the first row dims one in the last row of a tall column (19 segments away) under "+y", and the reverse under "-y"."""
    D, H, W = 3, 300, 5
    vol = np.zeros((D, H, W), np.float32)
    vol[1, 0, 2] = vol[1, H - 1, 2] = 2.0
    alpha, shadow = -np.expm1(-0.4 * 2.0), AMBIENT + (1 - AMBIENT) * np.exp(-0.9 * 2.0)
    for light, dim_row, lit_row in (("+y", H - 1, 0), ("-y", 0, H - 1)):
        img = render_volumes(_dev(vol), RenderSettings(0.4, 0.9, AMBIENT, 1.0, light)).cpu().numpy()
        assert np.count_nonzero(img) == 2
        np.testing.assert_allclose(img[lit_row, 2], alpha, rtol=1e-6)
        np.testing.assert_allclose(img[dim_row, 2], alpha * shadow, rtol=1e-6)


# ---- c. bit-level properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", LIGHTS)
def test_bit_level_properties(light):
    s = RenderSettings(0.5, 1.0, AMBIENT, 1.0, light)
    B, T, (D, H, W) = 2, 3, (5, 33, 36)
    big = _dev(density("dense", (B, T + 2, D + 1, H, W), seed=5))
    sl = big[:, 1:T + 1, :D]                                 # strided in both batch dimensions, each volume dense
    assert not sl.is_contiguous() and sl[0, 0].is_contiguous()
    img, tr = render_volumes(sl, s, transmittance=True)
    assert img.shape == tr.shape == (B, T, H, W)
    again, tr2 = render_volumes(sl, s, transmittance=True)
    assert torch.equal(img, again) and torch.equal(tr, tr2)                                  # call to call
    assert torch.equal(img, render_volumes(sl, s))                                           # with and without the transmittance
    dense = sl.contiguous()
    assert torch.equal(img, render_volumes(dense, s))                                        # strided slice = its contiguous copy
    flat = dense.view(B * T, D, H, W)
    whole = render_volumes(flat, s)
    assert torch.equal(whole.view(B, T, H, W), img)
    for i in range(B * T):                                                                   # volume i alone; the loop over B and T
        assert torch.equal(render_volumes(flat[i:i + 1], s)[0], whole[i])
        assert torch.equal(render_volumes(sl[i // T, i % T], s), img[i // T, i % T])
    out = torch.full((B, T, H, W), -1.0, device=DEV)
    ws = render_workspace(B * T, (D, H, W), light, DEV)
    assert render_volumes(dense, s, out=out, workspace=ws) is out and torch.equal(out, img)
    assert torch.equal(render_volumes(sl.transpose(0, 1), s), img.transpose(0, 1))           # batch strides in any order


# ---- d. simulator --------------------------------------------------------------------------------------------------------------------
def _sim(B=2):
    sim = SmokeSimulator3D((16, 64, 64), device=DEV, batch_size=B)
    sim.add_incense_source([(30, 25, 8), (40, 36, 5)], [1.5, 0.8])
    return sim


def test_simulate_frames_is_the_render_of_simulate_sequence():
    s = RenderSettings()
    a, b = _sim(), _sim()
    frames = a.simulate_frames(3, s, chunk=2)                 # chunks of 2 + 1 steps
    vols = b.simulate_sequence(3)
    assert frames.shape == (2, 3, 64, 64)
    assert torch.equal(frames, render_volumes(vols, s))
    assert float(frames.max()) > 0.05                         # there is smoke in the picture
    for k in ("u", "v", "w", "p", "density"):
        assert torch.equal(getattr(a.ns_solver, k), getattr(b.ns_solver, k)), k
    assert a.history_len == 0 and a.get_chaos_features(as_tensor=True) is None
    out = torch.empty(2, 3, 64, 64, device=DEV)
    c = _sim()
    assert c.simulate_frames(3, out=out, chunk=4) is out and torch.equal(out, frames)


def test_render_after_simulate_step_and_chaos_features_unchanged():
    sim, ref = _sim(), _sim()
    with pytest.raises(RuntimeError):
        sim.render()
    for _ in range(10):
        vol = sim.simulate_step()
        ref.simulate_step()
    img, T = sim.render(transmittance=True)
    want, wantT = render_volumes(vol, transmittance=True)
    assert img.shape == (2, 64, 64) and torch.equal(img, want) and torch.equal(T, wantT)
    assert torch.equal(sim.render(RenderSettings(light="+z")), render_volumes(vol, RenderSettings(light="+z")))
    assert torch.equal(sim.get_chaos_features(as_tensor=True), ref.get_chaos_features(as_tensor=True))
    assert torch.equal(sim.simulate_step(), ref.simulate_step())                             # and the next step is the same step
    single = SmokeSimulator3D((16, 64, 64), device=DEV)
    single.add_incense_source([(30, 25, 8)], [1.5])
    v1 = single.simulate_step()
    assert single.render().shape == (64, 64) and torch.equal(single.render(), render_volumes(v1))


# ---- e. dataset ----------------------------------------------------------------------------------------------------------------------
def test_rendered_dataset_is_the_render_of_the_volume_dataset():
    from smokephysai_amd.models import SmokePhysNet
    np.random.seed(11)
    rd = RenderedSmokeDataset(3, (16, 64, 64), sequence_length=12, sim_batch=2)
    np.random.seed(11)
    vd = SyntheticSmokeDataset3D(3, (16, 64, 64), sequence_length=12, sim_batch=2)
    assert len(rd) == len(vd) == 3
    for r, v in zip(rd.data, vd.data):
        assert r["sequence"].shape == (12, 64, 64)
        assert torch.equal(r["sequence"], render_volumes(v["sequence"], RenderSettings()))
        assert r["chaos_features"] == v["chaos_features"] and r["source_config"] == v["source_config"]
    item = rd[1]
    assert item["input"].shape == item["target"].shape == (1, 64, 64) and item["chaos_features"].shape == (3,)
    assert item["sequence"].shape == (12, 64, 64) and item["chaos_features"].dtype == torch.float32
    lit = RenderedSmokeDataset(1, (16, 64, 64), sequence_length=12, sim_batch=2, render={"light": "none", "sigma_view": 0.2})
    assert lit.render == RenderSettings(sigma_view=0.2, light="none")
    batch = torch.utils.data.default_collate([rd[i] for i in range(3)])
    torch.manual_seed(0)
    model = SmokePhysNet().to(DEV).eval()
    with torch.no_grad():
        out = model(batch["input"])
    assert out["reconstructed"].shape == (3, 1, 128, 128) and out["physics_features"].shape == (3, 3)
    for k in ("reconstructed", "physics_features", "latent_features"):
        assert torch.isfinite(out[k]).all(), k


def test_create_data_loaders_render_depth(tmp_path):
    np.random.seed(12)
    train, val = create_data_loaders(batch_size=2, num_train=2, num_val=1, grid_size=(64, 64), device=DEV, cache_dir=str(tmp_path),
                                     render_depth=16, render={"light": "+y"}, sim_batch=2, labels="host", sequence_length=12)
    assert isinstance(train.dataset, RenderedSmokeDataset) and train.dataset.grid_size == (16, 64, 64)
    assert train.dataset.render == RenderSettings(light="+y")
    b = next(iter(train))
    assert b["input"].shape == b["target"].shape == (2, 1, 64, 64) and b["chaos_features"].shape == (2, 3) and b["sequence"].shape == (2, 12, 64, 64)
    assert next(iter(val))["input"].shape == (1, 1, 64, 64)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert len(names) == 2 and all(".render16_" in n for n in names), names                  # a 2-D cache is never loaded, nor written


# ---- f. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = _lib.load()
    s = RenderSettings(light="+y")
    with pytest.raises(ValueError):
        render_volumes(torch.zeros(65, 8, 8, device=DEV), s)
    with pytest.raises(ValueError, match="dense"):
        render_volumes(torch.zeros(4, 40, 16, device=DEV)[:, :, ::2], s)
    with pytest.raises(ValueError, match="dense"):
        render_volumes(torch.zeros(2, 4, 40, 8, device=DEV)[:, :, :33], s)
    with pytest.raises(ValueError):
        render_volumes(torch.zeros(4, 40, 8, device=DEV, dtype=torch.float64), s)
    vol = torch.ones(2, 4, 40, 8, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        render_volumes(vol, s, workspace=torch.empty(16, device=DEV))
    with pytest.raises(ValueError):
        render_volumes(vol, s, out=torch.empty(2, 40, 9, device=DEV))
    # ... and the C entry point itself: the outputs keep their fill
    img = torch.full((2, 40, 8), -7.0, device=DEV)
    desc = s.desc()
    st = _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    need = L.smk_volume_render_workspace(2, 4, 40, 8, _lib.SMK_LIGHT_POS_Y)
    ws = torch.empty(need // 4, device=DEV)
    small = L.smk_volume_render(vol.data_ptr(), 4 * 40 * 8, 2, 4, 40, 8, C.byref(desc), img.data_ptr(), 320, None, 0, ws.data_ptr(), need - 4, st)
    assert small == _lib.SMK_ERR_INVALID and b"workspace" in L.smk_last_error()
    deep = torch.zeros(65 * 64, device=DEV)
    rc = L.smk_volume_render(deep.data_ptr(), 65 * 64, 1, 65, 8, 8, C.byref(desc), img.data_ptr(), 64, None, 0, ws.data_ptr(), need, st)
    assert rc == _lib.SMK_ERR_UNSUPPORTED and b"D <= 64" in L.smk_last_error()
    bad = _lib.SmkRenderDesc(0.1, 0.1, 0.25, 1.0, 7)
    assert L.smk_volume_render(vol.data_ptr(), 1280, 2, 4, 40, 8, C.byref(bad), img.data_ptr(), 320, None, 0, ws.data_ptr(), need, st) == _lib.SMK_ERR_INVALID
    assert L.smk_volume_render(vol.data_ptr(), 1279, 2, 4, 40, 8, C.byref(desc), img.data_ptr(), 320, None, 0, ws.data_ptr(), need, st) == _lib.SMK_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((img == -7.0).all())
    assert L.smk_volume_render(vol.data_ptr(), 1280, 2, 4, 40, 8, C.byref(desc), img.data_ptr(), 320, None, 0, ws.data_ptr(), need, st) == _lib.SMK_OK
    torch.cuda.synchronize()
    assert bool((img > 0).all())
