"""GPU test of the host-side checks that the four render entry points share (csrc/render.hip, render_check): smk_volume_render,
smk_volume_render_backward, smk_volume_render_orbit and smk_volume_render_camera refuse one table of faults with the same status, each
before any launch.

Setup: n = 2 volumes of (4, 40, 8) under light "+y".  40 rows are more than one segment of 16, so the front view wants a workspace as
well; the moving cameras render 2 views per volume.  Every output is filled with -7 and still holds -7 after all the refusals and a
synchronise.  Nothing here reaches the device before the one valid call that ends each case: a refused call launches nothing, which is
what is asserted.  The buffers behind the calls are larger than any call here could touch (the volumes and the gradient hold 65 planes,
the workspace 1 MiB), so a check that failed to refuse would show as a written output, not as a stray access."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from smokephysai_amd import _lib                                                                                   # noqa: E402

DEV = "cuda"
N, D, H, W, VIEWS = 2, 4, 40, 8, 2
HW, CELLS = H * W, D * H * W
ENTRIES = ("smk_volume_render", "smk_volume_render_backward", "smk_volume_render_orbit", "smk_volume_render_camera")


def _desc(sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light=_lib.SMK_LIGHT_POS_Y):
    return _lib.SmkRenderDesc(sigma_view, sigma_light, ambient, gain, light)


# the faults every entry point answers with SMK_ERR_INVALID: name -> the arguments of `call` that differ from a valid call
FAULTS = {
    "sigma_view < 0": dict(desc=_desc(sigma_view=-0.1)),
    "sigma_light < 0": dict(desc=_desc(sigma_light=-0.1)),
    "ambient > 1": dict(desc=_desc(ambient=1.5)),
    "gain = 0": dict(desc=_desc(gain=0.0)),
    "light = 7": dict(desc=_desc(light=7)),
    "light = -1": dict(desc=_desc(light=-1)),
    "volume pointer off by 2 bytes": dict(vol_offset=2),
    "vol_stride = D*H*W - 1": dict(vol_stride=CELLS - 1),
    "short image (gradient) stride": dict(image_stride=HW - 1),
    "short transmittance stride": dict(trans_stride=HW - 1),
    "null workspace, full size claimed": dict(null_workspace=True),
    "workspace 4 bytes short": dict(short=4),
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_shared_faults_are_refused_before_any_launch(entry):
    L = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    planes = N * (1 if entry in ENTRIES[:2] else VIEWS)
    vols = torch.ones(N * 65 * HW, device=DEV)
    image = torch.full((planes, H, W), -7.0, device=DEV)        # the backward reads these two as upstream gradients
    trans = torch.full((planes, H, W), -7.0, device=DEV)
    grad = torch.full((N * 65 * HW,), -7.0, device=DEV)         # the backward's output
    ws = torch.zeros(1 << 18, device=DEV)
    need = getattr(L, entry + "_workspace")(N, D, H, W, _lib.SMK_LIGHT_POS_Y)
    assert 0 < need <= ws.numel() * 4
    az = (C.c_double * (N * VIEWS))(0.0, 37.5, 90.0, -123.0)
    el = (C.c_double * (N * VIEWS))(0.0, 30.0, 90.0, -60.0)
    angles = {ENTRIES[0]: (), ENTRIES[1]: (), ENTRIES[2]: (az, VIEWS), ENTRIES[3]: (az, el, VIEWS)}[entry]

    def call(depth=D, desc=_desc(), vol_offset=0, vol_stride=None, image_stride=HW, trans_stride=HW, null_workspace=False, short=0):
        vol_stride = depth * HW if vol_stride is None else vol_stride
        tail = (None if null_workspace else ws.data_ptr(), need - short, st)
        head = (vols.data_ptr() + vol_offset, vol_stride, N, depth, H, W, C.byref(desc)) + angles
        if entry == "smk_volume_render_backward":
            return L.smk_volume_render_backward(*head, image.data_ptr(), image_stride, trans.data_ptr(), trans_stride, grad.data_ptr(),
                                                depth * HW, *tail)
        return getattr(L, entry)(*head, image.data_ptr(), image_stride, trans.data_ptr(), trans_stride, *tail)

    for name, fault in FAULTS.items():
        assert call(**fault) == _lib.SMK_ERR_INVALID, (entry, name, L.smk_last_error())
    assert call(depth=65) == _lib.SMK_ERR_UNSUPPORTED and b"D <= 64" in L.smk_last_error(), (entry, L.smk_last_error())
    torch.cuda.synchronize()
    outputs = (grad,) if entry == "smk_volume_render_backward" else (image, trans)
    assert all(bool((t == -7.0).all()) for t in outputs), entry
    if entry == "smk_volume_render_backward":                   # a valid call reads finite upstream gradients
        image.fill_(1.0)
        trans.fill_(0.5)
    assert call() == _lib.SMK_OK, (entry, L.smk_last_error())
    torch.cuda.synchronize()
    written = (grad[:N * CELLS],) if entry == "smk_volume_render_backward" else (image, trans)
    assert all(bool(torch.isfinite(t).all()) and bool((t != -7.0).all()) for t in written), entry
    assert bool((grad[N * CELLS:] == -7.0).all())
