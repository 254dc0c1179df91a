"""GPU tests of the orbit render (SPEC_3D.md section 10, "Orbit views"): smk_volume_render_orbit (csrc/render_orbit.hip) through
render_orbit, SmokeSimulator3D.render_orbit and PerturbationTester.viewpoint_test, against tests/render_orbit_oracle.py.

Shapes (the smallest that reach each path): (1,1,1); (3,5,7); (6,5,8), D + W even, for the exact quarter turn; (5,33,36), two strips of
columns; (24,70,64), several groups of rows and two full strips; (64,40,48), the depth limit; (16,64,130), five strips with a tail of two
columns and five chunks of samples.  Each with 2 different volumes, both densities, the four sigma pairs, the three lights and the
azimuths 0, 90, 180, 270, 37.5, -123, 200.25 and 720.001.

Bounds:
  image: 1e-4 max-norm relative per plane (conftest.rel_err) against the float64 rule, transmittance: 1e-4 absolute -- the project's bar.
      section 10's 1e-5 cannot be carried over: the sample positions are fp32 numbers up to W, and their rounding moves the bilinear
      weights; the float32 replay of the rule on the CPU is itself 4.5e-5 (image) / 1.7e-5 (transmittance) away from float64 at worst over
      these cases -- at (16,64,130), azimuth 720.001, where a weight of order 1e-3 is formed from a position of order D -- and 8.9e-6 over
      the cases of tests/test_render_orbit_host.py.
  and: the device's worst error over all these cases is at most 10 times the replay's worst over the same cases (section 10's margin
      for the device's exp and summation order); test_device_error_is_within_ten_times_the_replays prints both.  Measured on MI355X:
      image 4.54e-5, transmittance 1.71e-5 -- the replay's own figures.
  The float64 references and the replay of a shape are computed once (threads share its 32 volume-azimuth pairs) and left unchanged.
  everything stated as "equal" is bit for bit (torch.equal)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import rel_err                                                                                       # noqa: E402
from render_oracle import DENSITIES                                                                                # noqa: E402
from render_orbit_oracle import (AMBIENT, GPU_AZIMUTHS, GPU_SHAPES, ORBIT_LIGHTS, SIGMAS, orbit_replay_samples,      # noqa: E402
                                 orbit_samples_fp64, render_orbit_lights_fp64, replay_lights_from_samples, volumes)
from smokephysai_amd import _lib                                                                                   # noqa: E402
from smokephysai_amd.physics import (RenderSettings, SmokeSimulator3D, orbit_samples, orbit_workspace, render_orbit,  # noqa: E402
                                     render_volumes)

DEV = "cuda"
_REFERENCE, _DEVICE = {}, {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _reference_of_view(vol, phi):
    """One volume from one azimuth: {(sv, sl, light): (float64 image, float64 transmittance, replay image error, replay transmittance error)}."""
    s64 = orbit_samples_fp64(vol, phi)
    s32, A32 = orbit_replay_samples(vol, phi)
    res = {}
    for sv, sl in SIGMAS:
        images, T = render_orbit_lights_fp64(s64, sv, sl, AMBIENT, 1.0)
        got, gotT = replay_lights_from_samples(s32, A32, sv, sl, AMBIENT, 1.0)
        for light in ORBIT_LIGHTS:
            res[sv, sl, light] = (images[light], T, rel_err(got[light], images[light]), float(np.abs(gotT - T).max()))
    return res


def _reference(shape):
    """Computed once per shape and left unchanged: the volumes, the float64 images [2, 8, H, W] of every (kind, sigma pair, light), and the
    float32 replay's worst errors against them.  The 32 (volume, azimuth) pairs of a shape are independent: a few threads share them."""
    if shape not in _REFERENCE:
        vols = {kind: volumes(kind, shape) for kind in DENSITIES}
        V = len(GPU_AZIMUTHS)
        jobs = [(kind, i, k) for kind in DENSITIES for i in range(2) for k in range(V)]
        with ThreadPoolExecutor(max_workers=8) as pool:
            done = list(pool.map(lambda j: _reference_of_view(vols[j[0]][j[1]], GPU_AZIMUTHS[j[2]]), jobs))
        ref, worst_img, worst_T, where = {}, 0.0, 0.0, None
        for (kind, i, k), res in zip(jobs, done):
            for (sv, sl, light), (img, T, e, eT) in res.items():
                slot = ref.setdefault((kind, sv, sl, light), (np.empty((2, V) + shape[1:]), np.empty((2, V) + shape[1:])))
                slot[0][i, k], slot[1][i, k] = img, T
                if e > worst_img:
                    worst_img, where = e, (kind, sv, sl, light, i, GPU_AZIMUTHS[k])
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
                for light in ORBIT_LIGHTS:
                    img, T = render_orbit(vol, GPU_AZIMUTHS, RenderSettings(sv, sl, AMBIENT, 1.0, light), transmittance=True)
                    assert img.shape == T.shape == (2, len(GPU_AZIMUTHS)) + shape[1:]
                    img, T = img.cpu().numpy(), T.cpu().numpy()
                    want, wantT = r["ref"][kind, sv, sl, light]
                    for i in range(2):
                        for k in range(len(GPU_AZIMUTHS)):
                            e, eT = rel_err(img[i, k], want[i, k]), float(np.abs(T[i, k] - wantT[i, k]).max())
                            if e > worst_img:
                                worst_img, where = e, (kind, sv, sl, light, i, GPU_AZIMUTHS[k])
                            worst_T = max(worst_T, eT)
        _DEVICE[shape] = (worst_img, worst_T, where)
    return _DEVICE[shape]


# ---- a. against the fp64 oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=str)
def test_orbit_matches_the_fp64_rule(shape):
    e, eT, where = _device_errors(shape)
    rp, rpT = _reference(shape)["replay"]
    print(f"orbit {shape}: device worst image rel err {e:.2e} at {where}, transmittance abs err {eT:.2e}; fp32 replay {rp:.2e} / {rpT:.2e} at {_reference(shape)['replay_at']}")
    assert e <= 1e-4 and eT <= 1e-4, (shape, e, eT, where)


def test_device_error_is_within_ten_times_the_replays():
    dev = [_device_errors(s) for s in GPU_SHAPES]
    rep = [_reference(s)["replay"] for s in GPU_SHAPES]
    d_img, d_T = max(d[0] for d in dev), max(d[1] for d in dev)
    r_img, r_T = max(r[0] for r in rep), max(r[1] for r in rep)
    print(f"orbit, all cases: device image {d_img:.2e} / transmittance {d_T:.2e}; fp32 replay image {r_img:.2e} / transmittance {r_T:.2e}")
    assert d_img <= 10 * r_img and d_T <= 10 * r_T


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=str)
def test_azimuth_zero_is_render_volumes(shape):
    for kind in DENSITIES:
        vol = _dev(_reference(shape)["vols"][kind])
        for sv, sl in SIGMAS:
            for light in ORBIT_LIGHTS:
                s = RenderSettings(sv, sl, AMBIENT, 1.0, light)
                img, T = render_orbit(vol, 0.0, s, transmittance=True)
                want, wantT = render_volumes(vol, s, transmittance=True)
                assert img.shape == want.shape == (2,) + shape[1:]
                for i in range(2):
                    assert rel_err(img[i].cpu().numpy(), want[i].cpu().numpy()) <= 1e-4
                assert float((T - wantT).abs().max()) <= 1e-4
                if light == "none":                              # the samples are the voxels and the march is the same march
                    assert torch.equal(img, want) and torch.equal(T, wantT)


def test_exact_quarter_turn_reads_voxels():
    """(6,5,8), D + W even: at 90 degrees every sample is a voxel, so the unlit image is the front view of the volume with x in the role
    of depth: rho[z, y, x] -> rho'[x, y, D-1-z]."""
    vol = _dev(_reference((6, 5, 8))["vols"]["dense"])
    turned = vol.permute(0, 3, 2, 1).flip(-1).contiguous()
    s = RenderSettings(0.5, 1.0, AMBIENT, 1.0, "none")
    img, T = render_orbit(vol, [90.0, -270.0], s, transmittance=True)
    want, wantT = render_volumes(turned, s, transmittance=True)                     # [2, 5, 6]: the image of the turned volume is 6 wide
    S, D, W = orbit_samples(6, 8), 6, 8
    assert S == 10 and img.shape == (2, 2, 5, 8)
    for k in range(2):
        assert torch.equal(img[:, k, :, 1:7], want) and torch.equal(T[:, k, :, 1:7], wantT)     # columns 1..6 see z = 5..0
        assert not img[:, k, :, 0].any() and not img[:, k, :, 7].any() and bool((T[:, k, :, [0, 7]] == 1).all())


# ---- b. bit-level properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", ORBIT_LIGHTS)
def test_bit_level_properties(light):
    s = RenderSettings(0.5, 1.0, AMBIENT, 1.0, light)
    shape = (5, 33, 36)
    D, H, W = shape
    vol = _dev(_reference(shape)["vols"]["dense"])
    az = list(GPU_AZIMUTHS)
    img, T = render_orbit(vol, az, s, transmittance=True)
    again, T2 = render_orbit(vol, az, s, transmittance=True)
    assert torch.equal(img, again) and torch.equal(T, T2)                                    # call to call
    assert torch.equal(img, render_orbit(vol, az, s))                                        # with and without the transmittance
    for i in range(2):                                                                       # a volume alone = in the batch
        assert torch.equal(render_orbit(vol[i], az, s), img[i])
        assert torch.equal(render_orbit(vol[i:i + 1], az, s)[0], img[i])
    for k, phi in enumerate(az):                                                             # a view alone = among other azimuths
        one, oneT = render_orbit(vol, phi, s, transmittance=True)
        assert one.shape == (2, H, W) and torch.equal(one, img[:, k]) and torch.equal(oneT, T[:, k])
    assert torch.equal(render_orbit(vol, az[::-1], s), img.flip(1))
    assert torch.equal(render_orbit(vol, az * 3, s), torch.cat([img] * 3, dim=1))            # 48 planes: three launches of 16
    per = torch.tensor([az, az[::-1]], dtype=torch.float64)                                  # one list per volume (720.001 is no float32)
    mixed = render_orbit(vol, per, s)
    assert torch.equal(mixed[0], img[0]) and torch.equal(mixed[1], img[1].flip(0))
    assert torch.equal(render_orbit(vol, np.array([az, az]), s), img)
    assert torch.equal(render_orbit(vol, [37.5], s)[:, 0], render_orbit(vol, 37.5, s))
    assert torch.equal(render_orbit(vol, 720.0, s), render_orbit(vol, 0.0, s))
    # a strided batch, each volume dense (what SmokeSimulator3D keeps and simulate_frames renders from)
    big = torch.zeros(2, 3, D + 1, H, W, device=DEV)
    big[:, 1, :D] = vol
    sl = big[:, 1, :D]
    assert not sl.is_contiguous() and sl[0].is_contiguous()
    assert torch.equal(render_orbit(sl, az, s), img)
    assert torch.equal(render_orbit(big[1, 1, :D], az, s), img[1])        # one volume out of the middle of a buffer
    # out= and workspace= reuse
    out = torch.full((2, len(az), H, W), -1.0, device=DEV)
    ws = orbit_workspace(2, shape, light, DEV)
    assert (ws is None) == (light == "none")
    assert render_orbit(vol, az, s, out=out, workspace=ws) is out and torch.equal(out, img)
    out.fill_(-1.0)
    assert torch.equal(render_orbit(vol, az, s, out=out, workspace=ws), img)


# ---- c. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = _lib.load()
    s = RenderSettings(light="+y")
    with pytest.raises(ValueError, match=r"\+z"):
        render_orbit(torch.zeros(4, 8, 8, device=DEV), 10.0, RenderSettings(light="+z"))
    with pytest.raises(RuntimeError, match="no backward"):
        render_orbit(torch.zeros(4, 8, 8, device=DEV, requires_grad=True), 10.0, s)
    with torch.no_grad():                                                                    # ... which is about autograd, not the flag
        assert render_orbit(torch.zeros(4, 8, 8, device=DEV, requires_grad=True), 10.0, s).shape == (8, 8)
    with pytest.raises(ValueError):
        render_orbit(torch.zeros(65, 8, 8, device=DEV), 10.0, s)
    with pytest.raises(ValueError, match="dense"):
        render_orbit(torch.zeros(4, 40, 16, device=DEV)[:, :, ::2], 10.0, s)
    vol = torch.ones(2, 4, 40, 8, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        render_orbit(vol, 10.0, s, workspace=torch.empty(16, device=DEV))
    with pytest.raises(ValueError):
        render_orbit(vol, [10.0, 20.0], s, out=torch.empty(2, 40, 8, device=DEV))
    # ... and the C entry point itself: the outputs keep their fill
    img = torch.full((4, 40, 8), -7.0, device=DEV)
    tr = torch.full((4, 40, 8), -7.0, device=DEV)
    desc = s.desc()
    st = _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    need = L.smk_volume_render_orbit_workspace(2, 4, 40, 8, _lib.SMK_LIGHT_POS_Y)
    assert need == 2 * 4 * 40 * 8 * 4
    ws = torch.empty(need // 4, device=DEV)
    az = (C.c_double * 4)(0.0, 37.5, 90.0, -123.0)

    def call(vols=vol, stride=1280, D=4, d=desc, a=az, nbytes=need, H=40, W=8):
        return L.smk_volume_render_orbit(vols.data_ptr(), stride, 2, D, H, W, C.byref(d), a, 2, img.data_ptr(), 320, tr.data_ptr(), 320,
                                         ws.data_ptr(), nbytes, st)

    assert call(nbytes=need - 4) == _lib.SMK_ERR_INVALID and b"workspace" in L.smk_last_error()
    deep = torch.zeros(2 * 65 * 64, device=DEV)
    assert call(vols=deep, stride=65 * 64, D=65, H=8, W=8) == _lib.SMK_ERR_UNSUPPORTED and b"D <= 64" in L.smk_last_error()
    plus_z = _lib.SmkRenderDesc(0.1, 0.1, 0.25, 1.0, _lib.SMK_LIGHT_POS_Z)
    assert call(d=plus_z) == _lib.SMK_ERR_UNSUPPORTED and b"SMK_LIGHT_POS_Z" in L.smk_last_error()
    assert call(d=_lib.SmkRenderDesc(0.1, 0.1, 0.25, 1.0, 7)) == _lib.SMK_ERR_INVALID
    assert call(a=(C.c_double * 4)(0.0, float("nan"), 90.0, 1.0)) == _lib.SMK_ERR_INVALID and b"azimuth" in L.smk_last_error()
    assert call(stride=1279) == _lib.SMK_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((img == -7.0).all()) and bool((tr == -7.0).all())
    assert call() == _lib.SMK_OK
    torch.cuda.synchronize()
    assert bool((img >= 0).all()) and bool((tr > 0).all()) and bool((img[0] > 0).all())      # the front view; at 90 degrees the outer columns see past the 4 planes
    want, wantT = render_orbit(vol, [[0.0, 37.5], [90.0, -123.0]], s, transmittance=True)
    assert torch.equal(img.view(2, 2, 40, 8), want) and torch.equal(tr.view(2, 2, 40, 8), wantT)


# ---- d. simulator and evaluation -----------------------------------------------------------------------------------------------------
def test_simulator_render_orbit_is_render_orbit_of_the_emitted_volume():
    sim = SmokeSimulator3D((8, 32, 32), device=DEV, batch_size=2)
    sim.add_incense_source([(14, 12, 4), (20, 18, 3)], [1.5, 0.8])
    with pytest.raises(RuntimeError):
        sim.render_orbit(30.0)
    for _ in range(3):
        vol = sim.simulate_step()
    az = [0.0, 45.0, 90.0]
    img, T = sim.render_orbit(az, transmittance=True)
    want, wantT = render_orbit(vol, az, transmittance=True)
    assert img.shape == (2, 3, 32, 32) and torch.equal(img, want) and torch.equal(T, wantT)
    assert float(img.max()) > 0.01                                                           # there is smoke in the picture
    assert torch.equal(sim.render_orbit(45.0, RenderSettings(light="none")), render_orbit(vol, 45.0, RenderSettings(light="none")))
    assert torch.equal(sim.render_orbit(0.0, RenderSettings(light="none")), sim.render(RenderSettings(light="none")))
    single = SmokeSimulator3D((8, 32, 32), device=DEV)
    single.add_incense_source([(14, 12, 4)], [1.5])
    for _ in range(3):
        v1 = single.simulate_step()
    assert single.render_orbit(30.0).shape == (32, 32) and torch.equal(single.render_orbit(30.0), render_orbit(v1, 30.0))
    assert single.render_orbit(az).shape == (3, 32, 32) and torch.equal(single.render_orbit(az), render_orbit(v1, az))


def test_viewpoint_test():
    from smokephysai_amd.evaluation.perturbation_tests import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).to(DEV).eval()
    vols = _dev(volumes("sparse", (8, 64, 64)))[:, None]                                     # [2, 1, 8, 64, 64]
    tester = PerturbationTester(device=DEV)
    same = tester.viewpoint_test(model, vols, azimuths=(0, 360))
    assert set(same) == {"viewpoint_feature_stability", "viewpoint_feature_variance", "per_azimuth", "num_views"}
    print("viewpoint_test (0, 360):", same)
    assert same["num_views"] == 2 and set(same["per_azimuth"]) == {0.0, 360.0}
    assert same["viewpoint_feature_stability"] == 1.0 and same["viewpoint_feature_variance"] == 0.0
    ring = tester.viewpoint_test(model, vols, batch_size=5)                                  # the default ring, chunks that split a volume's views
    assert ring["num_views"] == 12 and list(ring["per_azimuth"]) == [float(a) for a in range(0, 360, 30)]
    assert ring["per_azimuth"][0.0] == 1.0 and -1.0 <= ring["viewpoint_feature_stability"] <= 1.0
    assert ring["viewpoint_feature_stability"] == pytest.approx(np.mean([ring["per_azimuth"][float(a)] for a in range(30, 360, 30)]), abs=1e-6)
    assert ring["viewpoint_feature_variance"] > 0.0                                          # the other side of the plume is another picture
    with pytest.raises(ValueError):
        tester.viewpoint_test(model, vols[:, 0])
