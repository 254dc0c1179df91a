"""GPU tests of the free-camera render (SPEC_3D.md section 10, "Free camera"): smk_volume_render_camera (csrc/render_camera.hip) through
render_camera, SmokeSimulator3D.render_camera and PerturbationTester.viewpoint_test(elevation=...), against tests/render_camera_oracle.py.

Shapes (the smallest that reach each path): (1,1,1); (3,5,7); (6,5,8), where the orbit's fringe shows; (5,33,36), a tile tail in both
image axes (two strips of 32 columns, the second of 4; 33 rows = four full workgroups of 8 and one wave with a single row); (24,70,64),
several workgroups of rows with a tail of 6 and two full strips; (64,40,48), the depth limit; (16,64,130), five strips with a tail of two
columns and ten chunks of 16 samples.  The kernel has one path (a wave per 32 x 2 pixels, chunks of 16 samples skipped by their brick), so
the list needs no further edge.  Each with 2 different volumes, both densities, the four sigma pairs, the three lights and the views
(azimuth, elevation) = (0,0), (37.5,30), (-123,-60), (200.25,12.5), (90,90), (0,-90), (720.001,45), (45,0.001).

Bounds:
  image: 1e-4 max-norm relative per plane (conftest.rel_err) against the float64 rule, transmittance: 1e-4 absolute -- the project's bar.
      The float32 replay of the rule on the CPU is itself 2.59e-5 (image) / 2.56e-5 (transmittance) away from float64 at worst over
      these cases, both at (16,64,130), sparse, sigma (4,8), view (720.001, 45).
  and: the device's worst error over all these cases is at most 10 times the replay's worst over the same cases;
      test_device_error_is_within_ten_times_the_replays prints both.  Measured on MI355X: image 2.59e-5, transmittance 2.56e-5, at the
      replay's own worst case -- the replay's figures to the digits shown.
  The float64 references and the replay of a shape are computed once (threads share its 16 kind-view pairs) and left unchanged.
  Everything stated as "equal" is bit for bit (torch.equal)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import rel_err                                                                                       # noqa: E402
from render_oracle import DENSITIES                                                                                # noqa: E402
from render_camera_oracle import (AMBIENT, CAMERA_LIGHTS, GPU_SHAPES, GPU_VIEWS, SIGMAS, reference_of_view, volumes)  # noqa: E402
from smokephysai_amd import _lib                                                                                   # noqa: E402
from smokephysai_amd.physics import (RenderSettings, SmokeSimulator3D, camera_samples, camera_workspace, render_camera,  # noqa: E402
                                     render_orbit, render_volumes)

DEV = "cuda"
AZ, EL = [v[0] for v in GPU_VIEWS], [v[1] for v in GPU_VIEWS]
_REFERENCE, _DEVICE = {}, {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _reference(shape):
    """Computed once per shape and left unchanged: the volumes, the float64 images [2, 8, H, W] of every (kind, sigma pair, light), and the
    float32 replay's worst errors against them.  The 16 (kind, view) pairs of a shape are independent: a few threads share them."""
    if shape not in _REFERENCE:
        vols = {kind: volumes(kind, shape) for kind in DENSITIES}
        V = len(GPU_VIEWS)
        jobs = [(kind, k) for kind in DENSITIES for k in range(V)]
        with ThreadPoolExecutor(max_workers=8) as pool:
            done = list(pool.map(lambda j: reference_of_view(list(vols[j[0]]), *GPU_VIEWS[j[1]]), jobs))
        ref, worst_img, worst_T, where = {}, 0.0, 0.0, None
        for (kind, k), per_volume in zip(jobs, done):
            for i, res in enumerate(per_volume):
                for (sv, sl, light), (img, T, e, eT) in res.items():
                    slot = ref.setdefault((kind, sv, sl, light), (np.empty((2, V) + shape[1:]), np.empty((2, V) + shape[1:])))
                    slot[0][i, k], slot[1][i, k] = img, T
                    if e > worst_img:
                        worst_img, where = e, (kind, sv, sl, light, i, GPU_VIEWS[k])
                    worst_T = max(worst_T, eT)
        _REFERENCE[shape] = {"vols": vols, "ref": ref, "replay": (worst_img, worst_T), "replay_at": where}
    return _REFERENCE[shape]


def _device_errors(shape):
    """The device's worst errors against the float64 rule over every case of `shape` (rendered once per shape)."""
    if shape not in _DEVICE:
        r = _reference(shape)
        worst_img, worst_T, where = 0.0, 0.0, None
        for kind in DENSITIES:
            vol = _dev(r["vols"][kind])
            for sv, sl in SIGMAS:
                for light in CAMERA_LIGHTS:
                    img, T = render_camera(vol, AZ, EL, RenderSettings(sv, sl, AMBIENT, 1.0, light), transmittance=True)
                    assert img.shape == T.shape == (2, len(GPU_VIEWS)) + shape[1:]
                    img, T = img.cpu().numpy(), T.cpu().numpy()
                    want, wantT = r["ref"][kind, sv, sl, light]
                    for i in range(2):
                        for k in range(len(GPU_VIEWS)):
                            e, eT = rel_err(img[i, k], want[i, k]), float(np.abs(T[i, k] - wantT[i, k]).max())
                            if e > worst_img:
                                worst_img, where = e, (kind, sv, sl, light, i, GPU_VIEWS[k])
                            worst_T = max(worst_T, eT)
        _DEVICE[shape] = (worst_img, worst_T, where)
    return _DEVICE[shape]


# ---- a. against the fp64 oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=str)
def test_camera_matches_the_fp64_rule(shape):
    e, eT, where = _device_errors(shape)
    rp, rpT = _reference(shape)["replay"]
    print(f"camera {shape}: device worst image rel err {e:.2e} at {where}, transmittance abs err {eT:.2e}; fp32 replay {rp:.2e} / {rpT:.2e} "
          f"at {_reference(shape)['replay_at']}")
    assert e <= 1e-4 and eT <= 1e-4, (shape, e, eT, where)


def test_device_error_is_within_ten_times_the_replays():
    dev = [_device_errors(s) for s in GPU_SHAPES]
    rep = [_reference(s)["replay"] for s in GPU_SHAPES]
    d_img, d_T = max(d[0] for d in dev), max(d[1] for d in dev)
    r_img, r_T = max(r[0] for r in rep), max(r[1] for r in rep)
    print(f"camera, all cases: device image {d_img:.2e} / transmittance {d_T:.2e}; fp32 replay image {r_img:.2e} / transmittance {r_T:.2e}")
    assert d_img <= 10 * r_img and d_T <= 10 * r_T


def test_top_view_is_the_front_view_of_the_rearranged_volume():
    """(6,8,8), D and H even: at (0, 90) every sample is a voxel, rho_s[s,y',x'] = rho[c_z + (y' - c_y), c_y - t, x'].  Image row y' sees
    plane z = y' - 1 (rows 0 and 7 look past the 6 planes), the ray runs from y = 7 down to 0: the front view of rho[z, y, x] ->
    rho'[7 - y, z, x]; and the light from above, which travels along the ray, is that view's "+z" light."""
    vol = _dev(_reference((6, 5, 8))["vols"]["dense"][:, :, :4, :]).repeat(1, 1, 2, 1).contiguous()      # [2, 6, 8, 8]
    vol[:, :, 4:] *= 0.5
    assert camera_samples(6, 8, 8) == 14
    turned = vol.permute(0, 2, 1, 3).flip(1).contiguous()                                    # [2, 8 (depth: y descending), 6 (rows: z), 8]
    for light, front in (("none", "none"), ("-y", "+z")):
        s = RenderSettings(0.5, 1.0, AMBIENT, 1.0, light)
        img, T = render_camera(vol, [0.0, 360.0], 90.0, s, transmittance=True)
        want, wantT = render_volumes(turned, RenderSettings(0.5, 1.0, AMBIENT, 1.0, front), transmittance=True)      # [2, 6, 8]
        assert img.shape == (2, 2, 8, 8)
        for k in range(2):
            for i in range(2):
                assert rel_err(img[i, k, 1:7].cpu().numpy(), want[i].cpu().numpy()) <= 1e-4
            assert float((T[:, k, 1:7] - wantT).abs().max()) <= 1e-4
            if light == "none":                                      # the samples are the voxels and the march is the same march
                assert torch.equal(img[:, k, 1:7], want) and torch.equal(T[:, k, 1:7], wantT)
            assert not img[:, k, 0].any() and not img[:, k, 7].any() and bool((T[:, k, [0, 7]] == 1).all())


def test_level_camera_is_close_to_the_orbit_and_not_dispatched_to_it():
    shape = (6, 5, 8)
    vol = _dev(_reference(shape)["vols"]["dense"])
    s = RenderSettings(0.5, 1.0, AMBIENT, 1.0, "none")
    cam, orb = render_camera(vol, -123.0, 0.0, s), render_orbit(vol, -123.0, s)
    diff = float((cam - orb).abs().max())
    print(f"level camera against render_orbit at {shape}, azimuth -123: {diff:.2e}")
    assert 1e-5 < diff < 1e-2                                        # the fringe the orbit's shorter ray drops (SPEC_3D.md section 10)
    front = render_volumes(vol, s)
    assert torch.equal(render_camera(vol, 0.0, 0.0, s), front)       # no fringe in front: the voxels, marched in the same order


# ---- b. bit-level properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", CAMERA_LIGHTS)
def test_bit_level_properties(light):
    s = RenderSettings(0.5, 1.0, AMBIENT, 1.0, light)
    shape = (5, 33, 36)
    D, H, W = shape
    vol = _dev(_reference(shape)["vols"]["dense"])
    img, T = render_camera(vol, AZ, EL, s, transmittance=True)
    again, T2 = render_camera(vol, AZ, EL, s, transmittance=True)
    assert torch.equal(img, again) and torch.equal(T, T2)                                    # call to call
    assert torch.equal(img, render_camera(vol, AZ, EL, s))                                   # with and without the transmittance
    for i in range(2):                                                                       # a volume alone = in the batch
        assert torch.equal(render_camera(vol[i], AZ, EL, s), img[i])
        assert torch.equal(render_camera(vol[i:i + 1], AZ, EL, s)[0], img[i])
    for k, (phi, theta) in enumerate(GPU_VIEWS):                                             # a view alone = among other views
        one, oneT = render_camera(vol, phi, theta, s, transmittance=True)
        assert one.shape == (2, H, W) and torch.equal(one, img[:, k]) and torch.equal(oneT, T[:, k])
    assert torch.equal(render_camera(vol, AZ[::-1], EL[::-1], s), img.flip(1))
    assert torch.equal(render_camera(vol, AZ * 3, EL * 3, s), torch.cat([img] * 3, dim=1))   # 48 planes: three launches of 16
    # [n, V] tables, one list per volume, for either angle (720.001 is no float32)
    az2, el2 = torch.tensor([AZ, AZ[::-1]], dtype=torch.float64), torch.tensor([EL, EL[::-1]], dtype=torch.float64)
    mixed = render_camera(vol, az2, el2, s)
    assert torch.equal(mixed[0], img[0]) and torch.equal(mixed[1], img[1].flip(0))
    assert torch.equal(render_camera(vol, np.array([AZ, AZ]), EL, s), img)
    assert torch.equal(render_camera(vol, AZ, np.array([EL, EL]), s), img)
    # a number against a sequence: paired by broadcasting
    ring = render_camera(vol, [0.0, 37.5, 200.25], 30.0, s)
    assert ring.shape == (2, 3, H, W) and torch.equal(ring[:, 1], img[:, 1])
    assert torch.equal(ring, render_camera(vol, [0.0, 37.5, 200.25], [30.0] * 3, s))
    tilt = render_camera(vol, 37.5, [30.0, -60.0], s)
    assert tilt.shape == (2, 2, H, W) and torch.equal(tilt[:, 0], img[:, 1])
    assert torch.equal(render_camera(vol, [37.5], 30.0, s)[:, 0], img[:, 1])
    assert torch.equal(render_camera(vol, 720.0, 12.5, s), render_camera(vol, 0.0, 12.5, s))
    # a strided batch, each volume dense (what SmokeSimulator3D keeps)
    big = torch.zeros(2, 3, D + 1, H, W, device=DEV)
    big[:, 1, :D] = vol
    sl = big[:, 1, :D]
    assert not sl.is_contiguous() and sl[0].is_contiguous()
    assert torch.equal(render_camera(sl, AZ, EL, s), img)
    assert torch.equal(render_camera(big[1, 1, :D], AZ, EL, s), img[1])   # one volume out of the middle of a buffer
    # out= and workspace= reuse
    out = torch.full((2, len(AZ), H, W), -1.0, device=DEV)
    ws = camera_workspace(2, shape, light, DEV)
    assert (ws is None) == (light == "none")
    assert render_camera(vol, AZ, EL, s, out=out, workspace=ws) is out and torch.equal(out, img)
    out.fill_(-1.0)
    assert torch.equal(render_camera(vol, AZ, EL, s, out=out, workspace=ws), img)


# ---- c. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = _lib.load()
    s = RenderSettings(light="+y")
    with pytest.raises(ValueError, match=r"\+z"):
        render_camera(torch.zeros(4, 8, 8, device=DEV), 10.0, 5.0, RenderSettings(light="+z"))
    with pytest.raises(RuntimeError, match="no backward"):
        render_camera(torch.zeros(4, 8, 8, device=DEV, requires_grad=True), 10.0, 5.0, s)
    with torch.no_grad():                                                                    # ... which is about autograd, not the flag
        assert render_camera(torch.zeros(4, 8, 8, device=DEV, requires_grad=True), 10.0, 5.0, s).shape == (8, 8)
    with pytest.raises(ValueError):
        render_camera(torch.zeros(65, 8, 8, device=DEV), 10.0, 5.0, s)
    with pytest.raises(ValueError, match="dense"):
        render_camera(torch.zeros(4, 40, 16, device=DEV)[:, :, ::2], 10.0, 5.0, s)
    vol = torch.ones(2, 4, 40, 8, device=DEV)
    poisoned = torch.full((2, 40, 8), -7.0, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        render_camera(vol, 10.0, 5.0, s, out=poisoned, workspace=torch.empty(16, device=DEV))
    with pytest.raises(ValueError, match=r"\[-90, 90\]"):
        render_camera(vol, 10.0, 90.5, s, out=poisoned)
    with pytest.raises(ValueError, match="finite"):
        render_camera(vol, float("nan"), 5.0, s, out=poisoned)
    with pytest.raises(ValueError):
        render_camera(vol, [10.0, 20.0], 5.0, s, out=poisoned)
    torch.cuda.synchronize()
    assert bool((poisoned == -7.0).all())
    # ... and the C entry point itself: the outputs keep their fill
    img = torch.full((4, 40, 8), -7.0, device=DEV)
    tr = torch.full((4, 40, 8), -7.0, device=DEV)
    desc = s.desc()
    st = _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    need = L.smk_volume_render_camera_workspace(2, 4, 40, 8, _lib.SMK_LIGHT_POS_Y)
    assert need == 2 * 4 * 40 * 8 * 4
    ws = torch.empty(need // 4, device=DEV)
    az = (C.c_double * 4)(0.0, 37.5, 90.0, -123.0)
    el = (C.c_double * 4)(0.0, 30.0, 90.0, -60.0)

    def call(vols=vol, stride=1280, D=4, d=desc, a=az, e=el, nbytes=need, H=40, W=8):
        return L.smk_volume_render_camera(vols.data_ptr(), stride, 2, D, H, W, C.byref(d), a, e, 2, img.data_ptr(), 320, tr.data_ptr(), 320,
                                          ws.data_ptr(), nbytes, st)

    assert call(nbytes=need - 4) == _lib.SMK_ERR_INVALID and b"workspace" in L.smk_last_error()
    deep = torch.zeros(2 * 65 * 64, device=DEV)
    assert call(vols=deep, stride=65 * 64, D=65, H=8, W=8) == _lib.SMK_ERR_UNSUPPORTED and b"D <= 64" in L.smk_last_error()
    plus_z = _lib.SmkRenderDesc(0.1, 0.1, 0.25, 1.0, _lib.SMK_LIGHT_POS_Z)
    assert call(d=plus_z) == _lib.SMK_ERR_UNSUPPORTED and b"SMK_LIGHT_POS_Z" in L.smk_last_error()
    assert call(d=_lib.SmkRenderDesc(0.1, 0.1, 0.25, 1.0, 7)) == _lib.SMK_ERR_INVALID
    assert call(a=(C.c_double * 4)(0.0, float("nan"), 90.0, 1.0)) == _lib.SMK_ERR_INVALID and b"azimuth" in L.smk_last_error()
    assert call(e=(C.c_double * 4)(0.0, 30.0, 90.001, 1.0)) == _lib.SMK_ERR_INVALID and b"elevation" in L.smk_last_error()
    assert call(e=(C.c_double * 4)(0.0, float("inf"), 9.0, 1.0)) == _lib.SMK_ERR_INVALID and b"elevation" in L.smk_last_error()
    assert call(stride=1279) == _lib.SMK_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((img == -7.0).all()) and bool((tr == -7.0).all())
    assert call() == _lib.SMK_OK
    torch.cuda.synchronize()
    assert bool((img >= 0).all()) and bool((tr > 0).all()) and bool((img[0] > 0).all())      # plane 0 is the front view
    want, wantT = render_camera(vol, [[0.0, 37.5], [90.0, -123.0]], [[0.0, 30.0], [90.0, -60.0]], s, transmittance=True)
    assert torch.equal(img.view(2, 2, 40, 8), want) and torch.equal(tr.view(2, 2, 40, 8), wantT)


# ---- d. simulator and evaluation -----------------------------------------------------------------------------------------------------
def test_simulator_render_camera_is_render_camera_of_the_emitted_volume():
    sim = SmokeSimulator3D((8, 32, 32), device=DEV, batch_size=2)
    sim.add_incense_source([(14, 12, 4), (20, 18, 3)], [1.5, 0.8])
    with pytest.raises(RuntimeError):
        sim.render_camera(30.0, 20.0)
    for _ in range(3):
        vol = sim.simulate_step()
    az, el = [0.0, 45.0, 90.0], [0.0, 30.0, 90.0]
    img, T = sim.render_camera(az, el, transmittance=True)
    want, wantT = render_camera(vol, az, el, transmittance=True)
    assert img.shape == (2, 3, 32, 32) and torch.equal(img, want) and torch.equal(T, wantT)
    assert float(img.max()) > 0.01                                                           # there is smoke in the picture
    none = RenderSettings(light="none")
    assert torch.equal(sim.render_camera(45.0, 30.0, none), render_camera(vol, 45.0, 30.0, none))
    single = SmokeSimulator3D((8, 32, 32), device=DEV)
    single.add_incense_source([(14, 12, 4)], [1.5])
    for _ in range(3):
        v1 = single.simulate_step()
    assert single.render_camera(30.0, 20.0).shape == (32, 32) and torch.equal(single.render_camera(30.0, 20.0), render_camera(v1, 30.0, 20.0))
    assert single.render_camera(az, 20.0).shape == (3, 32, 32) and torch.equal(single.render_camera(az, 20.0), render_camera(v1, az, 20.0))


def test_viewpoint_test_with_an_elevation():
    from smokephysai_amd.evaluation.perturbation_tests import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).to(DEV).eval()
    vols = _dev(volumes("sparse", (8, 64, 64)))[:, None]                                     # [2, 1, 8, 64, 64]
    tester = PerturbationTester(device=DEV)
    old = tester.viewpoint_test(model, vols, azimuths=(0, 90, 200))
    assert tester.viewpoint_test(model, vols, azimuths=(0, 90, 200), elevation=None) == old  # bit for bit: the same path
    assert set(old) == {"viewpoint_feature_stability", "viewpoint_feature_variance", "per_azimuth", "num_views"}
    up = tester.viewpoint_test(model, vols, elevation=30.0, batch_size=5)
    print("viewpoint_test (elevation 30):", up)
    assert set(up) == set(old) | {"elevation"} and up["elevation"] == 30.0 and up["num_views"] == 12
    assert list(up["per_azimuth"]) == [float(a) for a in range(0, 360, 30)] and up["per_azimuth"][0.0] == 1.0
    assert all(np.isfinite(v) for v in up["per_azimuth"].values())
    assert np.isfinite(up["viewpoint_feature_stability"]) and -1.0 <= up["viewpoint_feature_stability"] <= 1.0
    assert np.isfinite(up["viewpoint_feature_variance"]) and up["viewpoint_feature_variance"] > 0.0
    same = tester.viewpoint_test(model, vols, azimuths=(0, 360), elevation=-45)
    # the same view twice: identical frames, so identical features -- no variance, and a cosine of 1 to the few fp32 roundings
    # (2^-24 each) of a dot product over two norms
    assert same["viewpoint_feature_variance"] == 0.0 and same["elevation"] == -45.0
    assert same["viewpoint_feature_stability"] == pytest.approx(1.0, abs=1e-6)
