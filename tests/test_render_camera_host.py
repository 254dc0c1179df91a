"""CPU tests of the free-camera render (SPEC_3D.md section 10, "Free camera"): the properties of the numpy oracle
(tests/render_camera_oracle.py) that pin the rule -- the orbit's samples at elevation 0, the fringe that makes the images differ, the top
view, the identities, the sample count, the angle rule --, the fp32 error budget the device tolerance is derived from, and the
host-side surface of render_camera, camera_supported, camera_samples, camera_workspace and viewpoint_test(elevation=...).  No GPU.

fp32 budget: the float32 replay of the rule stays within 1e-4 of the float64 rule (the project's bar) over both case lists of the
oracle, each with 2 volumes, both densities, the four sigma pairs and the three lights.  Measured (printed by the test, recorded in
SPEC_3D.md section 10): GPU_SHAPES x GPU_VIEWS image 2.59e-5, transmittance 2.56e-5, both at (16,64,130), sparse, view (720.001, 45);
HOST_SHAPES x HOST_VIEWS image 6.12e-5, transmittance 4.42e-5 at (5,33,36), dense, view (200.25, 89.999)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from render_oracle import DENSITIES, light_prefix, render_fp64
from render_orbit_oracle import orbit_samples_count, orbit_samples_fp64, render_orbit_fp64
from render_camera_oracle import (AMBIENT, CAMERA_LIGHTS, GPU_SHAPES, GPU_VIEWS, HOST_SHAPES, HOST_VIEWS, SIGMAS, camera_coefficients,
                                  camera_grid, camera_light_samples_fp64, camera_lights_fp64, camera_replay_samples, camera_samples_count,
                                  camera_samples_fp64, density, reference_of_view, render_camera_fp32_replay, render_camera_fp64,
                                  replay_lights_from_samples)

OBLIQUE = ((37.5, 30.0), (-123.0, -60.0), (200.25, 12.5), (90.001, 89.999), (311.0, -45.0))


# ---- 1, 2: elevation 0 has the orbit's samples on a longer ray, and not the orbit's image ------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 33, 36), (6, 5, 8), (4, 40, 6)], ids=str)
def test_level_camera_has_the_orbits_samples_in_the_middle_of_its_ray(shape):
    rho = density("dense", shape, seed=1).astype(np.float64)
    S, So = camera_samples_count(*shape), orbit_samples_count(shape[0], shape[2])
    assert S >= So and (S - So) % 2 == 0
    pad = (S - So) // 2
    for phi in (0.0, 90.0, 37.5, -123.0):
        cam, orb = camera_samples_fp64(rho, phi, 0.0), orbit_samples_fp64(rho, phi)
        assert cam.shape == (S,) + shape[1:]
        assert np.abs(cam[pad:pad + So] - orb).max() == 0.0


def test_level_camera_is_not_the_orbit_image():
    """(6,5,8) at azimuth -123: the orbit's shorter ray drops fringe samples whose bilinear footprint still touches a corner voxel, so
    elevation 0 is a rule of its own (render_camera must not dispatch to the orbit kernel)."""
    rho = density("dense", (6, 5, 8), seed=1).astype(np.float64)
    cam = camera_samples_fp64(rho, -123.0, 0.0)
    So = orbit_samples_count(6, 8)
    pad = (cam.shape[0] - So) // 2
    assert pad > 0 and (cam[:pad].any() or cam[pad + So:].any())                     # smoke the orbit's ray does not reach
    img, T = render_camera_fp64(rho, -123.0, 0.0, 0.5, 1.0, AMBIENT, 1.0, "none")
    orb, orbT = render_orbit_fp64(rho, -123.0, 0.5, 1.0, AMBIENT, 1.0, "none")
    diff = np.abs(img - orb).max()
    print(f"level camera against the orbit at (6,5,8), azimuth -123: {diff:.2e}")
    assert 1e-5 < diff < 1e-2
    img0, _ = render_camera_fp64(rho, 0.0, 0.0, 0.5, 1.0, AMBIENT, 1.0, "none")      # the front view has no fringe: the images agree
    assert np.abs(img0 - render_fp64(rho, 0.5, 1.0, AMBIENT, 1.0, "none")[0]).max() <= 1e-12


# ---- 3: the top view ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7), (6, 8, 8), (5, 33, 36)], ids=str)
def test_top_view_lands_on_voxel_centres_when_d_and_h_have_one_parity(shape):
    D, H, W = shape
    assert (D - H) % 2 == 0
    rho = density("dense", shape, seed=2).astype(np.float64)
    S = camera_samples_count(*shape)
    cz, cy, tc = (D - 1) / 2, (H - 1) / 2, (S - 1) / 2
    want = np.zeros((S, H, W))
    for s in range(S):
        for yp in range(H):
            z, y = cz + (yp - cy), cy - (s - tc)
            assert z == int(z) and y == int(y)
            if 0 <= z < D and 0 <= y < H:
                want[s, yp] = rho[int(z), int(y)]
    assert np.abs(camera_samples_fp64(rho, 0.0, 90.0) - want).max() == 0.0
    for sv, sl in SIGMAS:
        img, T = render_camera_fp64(rho, 0.0, 90.0, sv, sl, AMBIENT, 1.3, "none")
        w, wT = render_fp64(want, sv, sl, AMBIENT, 1.3, "none")
        assert np.abs(img - w).max() == 0.0 and np.abs(T - wT).max() == 0.0
        # the light from above travels along the ray: "-y" is the rearranged array's "+z"
        img, _ = render_camera_fp64(rho, 0.0, 90.0, sv, sl, AMBIENT, 1.3, "-y")
        assert np.abs(img - render_fp64(want, sv, sl, AMBIENT, 1.3, "+z")[0]).max() <= 1e-12
    below = camera_samples_fp64(rho, 0.0, -90.0)                      # from below: the same voxels, rows mirrored, in reverse order
    assert np.abs(below - want[::-1, ::-1]).max() == 0.0


# ---- 4, 5, 6: identities at every view ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7), (6, 5, 8), (5, 9, 12), (8, 4, 3)], ids=str)
def test_identities_at_every_view(shape):
    for kind in DENSITIES:
        rho = density(kind, shape, seed=5)
        for phi, theta in OBLIQUE + ((0.0, 0.0), (90.0, 90.0), (0.0, -90.0)):
            grid = camera_grid(shape, phi, theta)
            rs = camera_samples_fp64(rho, phi, theta, grid)
            As = camera_light_samples_fp64(rho, phi, theta, grid=grid)
            assert rs.min() >= 0.0 and all(A.min() >= 0.0 for A in As.values())
            for sv, sl in SIGMAS:
                images, T = camera_lights_fp64(rs, As, sv, sl, AMBIENT, 1.0)
                assert np.abs(images["none"] + T - 1.0).max() <= 1e-12                        # unlit, gain 1: what is not transmitted is seen
                for g in (1.0, 2.5):
                    images, T = camera_lights_fp64(rs, As, sv, sl, AMBIENT, g)
                    for light in CAMERA_LIGHTS:
                        assert images[light].min() >= 0.0 and (images[light] - g * (1.0 - T)).max() <= 1e-12
    empty = np.zeros(shape, np.float32)
    for phi, theta in OBLIQUE:
        for light in CAMERA_LIGHTS:
            img, T = render_camera_fp64(empty, phi, theta, 0.5, 1.0, AMBIENT, 1.0, light)
            assert not img.any() and np.array_equal(T, np.ones(shape[1:]))


def test_one_call_forms_equal_the_shared_forms():
    rho = density("dense", (5, 9, 12), seed=7)
    for phi, theta in ((0.0, 0.0), (37.5, 30.0), (200.25, -77.0)):
        grid = camera_grid(rho.shape, phi, theta)
        rs, As = camera_samples_fp64(rho, phi, theta, grid), camera_light_samples_fp64(rho, phi, theta, grid=grid)
        for light in ("+y", "-y"):                                   # A_s is the interpolation of the voxel-grid prefix, by definition
            assert np.array_equal(As[light], grid.interpolate(np.ascontiguousarray(light_prefix(rho.astype(np.float64), light))))
        for sv, sl in SIGMAS:
            images, T = camera_lights_fp64(rs, As, sv, sl, AMBIENT, 1.7)
            for light in CAMERA_LIGHTS:
                want, wantT = render_camera_fp64(rho, phi, theta, sv, sl, AMBIENT, 1.7, light)
                assert np.array_equal(images[light], want) and np.array_equal(T, wantT)
    got, gotT = render_camera_fp32_replay(rho, 37.5, 30.0, 0.1, 0.1, AMBIENT, 1.0, "-y")
    rs32, A32 = camera_replay_samples(rho, 37.5, 30.0)
    want, wantT = replay_lights_from_samples(rs32, A32, 0.1, 0.1, AMBIENT, 1.0)
    assert np.array_equal(got, want["-y"]) and np.array_equal(gotT, wantT) and got.dtype == np.float32
    with pytest.raises(ValueError):
        render_camera_fp64(rho, 0.0, 0.0, light="+z")


def test_pitched_prefix_is_not_the_prefix_of_the_samples():
    """With pitch the interpolation acts along y too: the sampled prefix is the definition, not a prefix of the samples."""
    rho = density("dense", (5, 9, 12), seed=6).astype(np.float64)
    rs, As = camera_samples_fp64(rho, 37.5, 30.0), camera_light_samples_fp64(rho, 37.5, 30.0)
    assert np.abs(light_prefix(rs, "+y") - As["+y"]).max() > 1e-3
    level = camera_light_samples_fp64(rho, 37.5, 0.0)["+y"]          # level: the orbit's statement holds
    assert np.abs(light_prefix(camera_samples_fp64(rho, 37.5, 0.0), "+y") - level).max() <= 1e-12


# ---- S and the angle rule ----------------------------------------------------------------------------------------------------------------
def test_sample_count_covers_the_diagonal_with_the_parity_of_d():
    from smokephysai_amd.physics import camera_samples
    for D, H, W in set(GPU_SHAPES + HOST_SHAPES + [(64, 1, 1024), (1, 1024, 1), (64, 1024, 1024), (2, 3, 6), (1, 65536, 1)]):
        S = camera_samples_count(D, H, W)
        assert S == camera_samples(D, H, W)
        assert S * S >= D * D + H * H + W * W and (S - D) % 2 == 0 and (S < 2 or (S - 2) ** 2 < D * D + H * H + W * W)
    assert camera_samples_count(2, 3, 6) == 8 and camera_samples_count(1, 2, 2) == 3 and camera_samples_count(1, 1, 1) == 3
    assert camera_samples_count(3, 5, 7) == 11 and camera_samples_count(16, 64, 130) == 146
    with pytest.raises(ValueError):
        camera_samples(0, 1, 1)


def test_angle_rule():
    f = np.float32
    one, zero = f(1), f(0)
    assert camera_coefficients(0, 0) == ((one, zero, zero), (zero, one, zero), (zero, zero, one))     # the front view: x, y, +z
    assert camera_coefficients(720.0, 0) == camera_coefficients(0, 0)
    r, e, d = camera_coefficients(0, 90)                             # the top view: rows run along z, the ray runs down
    assert r == (one, zero, zero) and e == (zero, zero, one) and d == (zero, -one, zero)
    r, e, d = camera_coefficients(0, -90)
    assert e == (zero, zero, -one) and d == (zero, one, zero)
    r, e, d = camera_coefficients(90, 0)                             # the orbit's quarter turn
    assert r == (zero, zero, -one) and e == (zero, one, zero) and d == (one, zero, zero)
    r, e, d = camera_coefficients(37.5, 30.0)
    c, s = float(f(np.cos(np.radians(37.5)))), float(f(np.sin(np.radians(37.5))))
    ce, se = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    assert r == (f(c), zero, f(-s)) and e == (f(s * se), f(ce), f(c * se)) and d == (f(s * ce), f(-se), f(c * ce))
    assert d[1] < 0 and e[1] > 0                                     # a raised camera looks down; up keeps pointing up
    assert all(v.dtype == np.float32 for t in camera_coefficients(200.25, -12.5) for v in t)
    r, e, d = camera_coefficients(10.0, 89.999)                      # close to the top is not the top
    assert e[1] != zero and abs(float(e[1]) - np.radians(0.001)) < 1e-9
    for t in (camera_coefficients(37.5, 30.0), camera_coefficients(-123.0, -60.0)):                   # an orthonormal frame, to fp32
        m = np.array(t, np.float64)
        assert np.abs(m @ m.T - np.eye(3)).max() < 1e-6
    for bad in ((0, 90.001), (0, -91), (0, float("nan")), (float("inf"), 0)):
        with pytest.raises(ValueError):
            camera_coefficients(*bad)


# ---- the fp32 budget ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cases", ["host", "gpu"])
def test_fp32_replay_stays_within_the_bar(cases):
    shapes, views = (HOST_SHAPES, HOST_VIEWS) if cases == "host" else (GPU_SHAPES, GPU_VIEWS)
    jobs = [(shape, kind, view) for shape in shapes for kind in DENSITIES for view in views]

    def worst_of(job):
        shape, kind, view = job
        res = reference_of_view([density(kind, shape, seed=i) for i in range(2)], *view)
        return max(r[k][2] for r in res for k in r), max(r[k][3] for r in res for k in r)

    with ThreadPoolExecutor(max_workers=8) as pool:
        done = list(pool.map(worst_of, jobs))
    k = int(np.argmax([d[0] for d in done]))
    kT = int(np.argmax([d[1] for d in done]))
    print(f"camera replay, {cases} cases: worst image rel err {done[k][0]:.2e} at {jobs[k]}, worst transmittance abs err {done[kT][1]:.2e} "
          f"at {jobs[kT]}")
    assert done[k][0] <= 1e-4 and done[kT][1] <= 1e-4


# ---- the Python surface, as far as it needs no device -----------------------------------------------------------------------------------
def test_argument_checks_that_need_no_device():
    from smokephysai_amd.physics import RenderSettings, camera_supported, camera_workspace, render_camera
    vols = torch.zeros(2, 4, 6, 8)
    with pytest.raises(ValueError, match=r"\+z"):
        render_camera(vols, 30.0, 10.0, RenderSettings(light="+z"))
    with pytest.raises(ValueError, match=r"\+z"):
        camera_workspace(1, (4, 6, 8), "+z", "cpu")
    for bad in ([[0.0, 1.0, 2.0]], [[0.0], [1.0], [2.0]], [], np.zeros((2, 2, 2)), "front", None, True):
        with pytest.raises(ValueError, match="azimuth"):
            render_camera(vols, bad, 0.0)
        with pytest.raises(ValueError, match="elevation"):
            render_camera(vols, 0.0, bad)
    for bad in (float("nan"), [0.0, float("inf")], torch.tensor([[0.0, float("nan")], [1.0, 2.0]])):
        with pytest.raises(ValueError, match="finite"):
            render_camera(vols, bad, 0.0)
        with pytest.raises(ValueError, match="finite"):
            render_camera(vols, 0.0, bad)
    for bad in (90.001, -91.0, [0.0, 120.0], torch.tensor([[0.0, 10.0], [-90.5, 2.0]])):
        with pytest.raises(ValueError, match=r"\[-90, 90\]"):
            render_camera(vols, 0.0, bad)
    with pytest.raises(ValueError, match="paired"):                                  # two sequences have one V
        render_camera(vols, [0.0, 10.0, 20.0], [0.0, 10.0])
    with pytest.raises(ValueError, match="paired"):
        render_camera(vols, np.zeros((2, 3)), [0.0, 10.0])
    with pytest.raises(ValueError):
        render_camera(torch.zeros(2, 3, 4, 6, 8), 0.0, 0.0)       # [B,T,D,H,W] is render_volumes' form, not this one's
    with pytest.raises(ValueError):
        render_camera(vols.double(), 0.0, 0.0)
    with pytest.raises(TypeError):
        render_camera(vols, 0.0, 0.0, {"light": "none"})
    with pytest.raises(RuntimeError, match="no backward"):
        render_camera(vols.clone().requires_grad_(), 0.0, 0.0)
    for az, el in ((0.0, 0.0), ([0.0, 90.0], 30.0), (10.0, [0.0, 90.0]), (np.zeros((2, 3)), [0.0, 1.0, 2.0]), (torch.zeros(2, 1), 90.0),
                   ([1.0, 2.0], torch.zeros(2, 2)), (0, -90)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):                   # every valid form reaches the device check
            render_camera(vols, az, el)
    assert camera_supported(1, 1, 1) and camera_supported(64, 40, 1024) and camera_supported(64, 1024, 1024) and camera_supported(2, 65536, 8)
    assert not camera_supported(65, 8, 8) and not camera_supported(0, 8, 8) and not camera_supported(8, 8, 1025)
    assert not camera_supported(1, 65537, 1) and not camera_supported(64, 32768, 1024) and not camera_supported(8, 0, 8)
    with pytest.raises(TypeError):
        camera_supported(8.0, 8, 8)


def test_angle_forms_broadcast_against_each_other():
    from smokephysai_amd.physics.render import _camera_angles
    az, el, views = _camera_angles(10.0, -20.0, 3)
    assert not views and az.tolist() == [[10.0]] * 3 and el.tolist() == [[-20.0]] * 3
    az, el, views = _camera_angles([0.0, 90.0], 30.0, 2)
    assert views and az.tolist() == [[0.0, 90.0]] * 2 and el.tolist() == [[30.0, 30.0]] * 2
    az, el, views = _camera_angles(45.0, [0.0, 30.0, 90.0], 2)
    assert views and az.tolist() == [[45.0] * 3] * 2 and el.tolist() == [[0.0, 30.0, 90.0]] * 2
    az, el, views = _camera_angles([1.0, 2.0], [[10.0, 20.0], [30.0, 40.0]], 2)                     # paired, not a product
    assert views and az.tolist() == [[1.0, 2.0], [1.0, 2.0]] and el.tolist() == [[10.0, 20.0], [30.0, 40.0]]
    az, el, views = _camera_angles(torch.tensor([[720.001], [5.0]], dtype=torch.float64), 7.0, 2)
    assert views and az.tolist() == [[720.001], [5.0]] and el.tolist() == [[7.0], [7.0]] and az.dtype == el.dtype == torch.float64
    az, el, views = _camera_angles([5.0], 7.0, 1)                                                    # a sequence of one is still a sequence
    assert views and az.shape == el.shape == (1, 1)


def test_exports():
    import dataclasses

    from smokephysai_amd import _lib, physics
    assert [f.name for f in dataclasses.fields(physics.RenderSettings)] == ["sigma_view", "sigma_light", "ambient", "gain", "light"]
    for name in ("render_camera", "camera_supported", "camera_samples", "camera_workspace"):
        assert name in physics.__all__ and callable(getattr(physics, name))
    L = _lib.load()
    assert "smk_volume_render_camera" in _lib.EXPORTS and "smk_volume_render_camera_workspace" in _lib.EXPORTS
    assert L.smk_abi_version() == 17
    assert L.smk_volume_render_camera_workspace(2, 4, 6, 8, _lib.SMK_LIGHT_NONE) == 0
    assert L.smk_volume_render_camera_workspace(2, 4, 6, 8, _lib.SMK_LIGHT_NEG_Y) == 2 * 4 * 6 * 8 * 4
    assert L.smk_volume_render_camera_workspace(2, 4, 6, 8, _lib.SMK_LIGHT_POS_Z) == -1
    assert L.smk_volume_render_camera_workspace(2, 65, 6, 8, _lib.SMK_LIGHT_NONE) == -1
    assert L.smk_volume_render_camera_workspace(2, 4, 6, 1025, _lib.SMK_LIGHT_NONE) == -1
    assert L.smk_volume_render_camera_workspace(1, 1, 65537, 1, _lib.SMK_LIGHT_NONE) == -1
    assert L.smk_volume_render_camera_workspace(1, 64, 1024, 1024, _lib.SMK_LIGHT_POS_Y) == 64 * 1024 * 1024 * 4
    assert hasattr(physics.SmokeSimulator3D, "render_camera")


# ---- viewpoint_test: None is the old path ------------------------------------------------------------------------------------------------
def test_viewpoint_test_elevation_none_takes_the_orbit_path(monkeypatch):
    from smokephysai_amd import physics
    from smokephysai_amd.evaluation.perturbation_tests import PerturbationTester
    calls = []

    def fake_orbit(vols, azimuth, settings=None, **kw):
        calls.append(("orbit", tuple(azimuth), settings))
        return torch.stack([torch.full((vols.shape[0], 8, 8), float(k)) for k in range(len(azimuth))], dim=1)

    def fake_camera(vols, azimuth, elevation, settings=None, **kw):
        calls.append(("camera", tuple(azimuth), elevation, settings))
        return torch.stack([torch.full((vols.shape[0], 8, 8), float(k)) for k in range(len(azimuth))], dim=1)

    class Model(torch.nn.Module):
        def forward(self, x):
            return {"physics_features": torch.stack([x.mean(dim=(1, 2, 3)) + 1.0, torch.ones(x.shape[0])], dim=1)}

    monkeypatch.setattr(physics, "render_orbit", fake_orbit)
    monkeypatch.setattr(physics, "render_camera", fake_camera)
    tester = PerturbationTester(device="cpu")
    vols = torch.zeros(2, 1, 4, 8, 8)
    old = tester.viewpoint_test(Model(), vols, azimuths=(0, 120, 240))
    assert calls == [("orbit", (0.0, 120.0, 240.0), None)]
    assert set(old) == {"viewpoint_feature_stability", "viewpoint_feature_variance", "per_azimuth", "num_views"} and old["num_views"] == 3
    assert tester.viewpoint_test(Model(), vols, azimuths=(0, 120, 240), elevation=None) == old and calls[-1][0] == "orbit"
    new = tester.viewpoint_test(Model(), vols, azimuths=(0, 120, 240), elevation=30)
    assert calls[-1] == ("camera", (0.0, 120.0, 240.0), 30.0, None) and len(calls) == 3              # one render_camera call
    assert set(new) == set(old) | {"elevation"} and new["elevation"] == 30.0 and new["num_views"] == 3
    assert {k: new[k] for k in old} == old                                                           # the same frames, the same figures
    with pytest.raises(ValueError, match="elevation"):
        tester.viewpoint_test(Model(), vols, elevation="high")
    with pytest.raises(TypeError):
        tester.viewpoint_test(Model(), vols, (0, 90), None, 64, 30.0)                                # keyword-only
