"""CPU-side checks of the Lyapunov spectrum's summaries (smokephysai_amd/physics/fluid_tangent.py): the four new symbols
are declared, exported and bound and refuse what they must without touching anything; kaplan_yorke_dimension and ks_entropy on hand-made
spectra; the gram_schmidt keyword is checked; flow_chaos(route="torch") is lyapunov_exponents(k=4, route="torch") plus the two formulas."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step_grad_oracle as O                                                                      # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd.physics import (FlowChaos, flow_chaos, flow_chaos3d, kaplan_yorke_dimension, ks_entropy,        # noqa: E402
                                     lyapunov_exponents, lyapunov_exponents3d)

NEW = ("smk_tangent_orthonormalize", "smk_tangent_orthonormalize_workspace", "smk_tangent3d_orthonormalize",
       "smk_tangent3d_orthonormalize_workspace")


def test_the_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/smokehip.h"
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib._SIGNATURES["smk_tangent_orthonormalize"] == _lib._SIGNATURES["smk_tangent_renorm"]
    assert _lib._SIGNATURES["smk_tangent3d_orthonormalize"] == _lib._SIGNATURES["smk_tangent3d_renorm"]
    assert L.smk_tangent_orthonormalize_workspace.restype is _lib.C.c_int64
    assert L.smk_tangent3d_orthonormalize_workspace.restype is _lib.C.c_int64
    import smokephysai_amd.physics as physics
    for name in ("FlowChaos", "flow_chaos", "flow_chaos3d", "kaplan_yorke_dimension", "ks_entropy"):
        assert name in physics.__all__ and hasattr(physics, name)
    assert hasattr(physics.SmokeSimulator, "flow_chaos") and hasattr(physics.SmokeSimulator3D, "flow_chaos")


def test_the_workspace_queries_follow_the_renorm_queries_up_to_eight_vectors():
    L = _lib.load()
    for T in (1, 2, 3, 8):
        assert L.smk_tangent_orthonormalize_workspace(2, T, 33, 40) == L.smk_tangent_renorm_workspace(2, T, 33, 40) > 0
        assert L.smk_tangent3d_orthonormalize_workspace(2, T, 6, 9, 12) == L.smk_tangent3d_renorm_workspace(2, T, 6, 9, 12) > 0
    assert L.smk_tangent_renorm_workspace(2, 9, 33, 40) > 0
    for B, T, H, W in ((2, 9, 33, 40), (0, 1, 8, 8), (1, 0, 8, 8), (65535, 2, 8, 8), (1, 1, 2, 8), (1, 1, 8, 2), (1, 1, 32767, 8)):
        assert L.smk_tangent_orthonormalize_workspace(B, T, H, W) == -1, (B, T, H, W)
    for B, T, D, H, W in ((2, 9, 6, 9, 12), (0, 1, 8, 8, 8), (1, 0, 8, 8, 8), (1, 1, 2, 8, 8), (1000, 8, 8, 8, 8)):
        assert L.smk_tangent3d_orthonormalize_workspace(B, T, D, H, W) == -1, (B, T, D, H, W)


def test_the_entry_points_refuse_bad_arguments_before_touching_anything():
    L = _lib.load()
    one = 4096                   # never dereferenced: every call below is refused on its arguments
    two, three = L.smk_tangent_orthonormalize, L.smk_tangent3d_orthonormalize
    assert two(one, one, one, one, one, 2, 9, 8, 8, 8, 9, one, 1 << 30, None) == _lib.SMK_ERR_INVALID
    assert "T <= 8" in L.smk_last_error().decode()
    assert two(one, one, one, one, one, 2, 3, 8, 8, 7, 9, one, 1 << 30, None) == _lib.SMK_ERR_INVALID
    assert two(one, one, one, one, one, 2, 3, 8, 8, 8, 9, one, L.smk_tangent_orthonormalize_workspace(2, 3, 8, 8) - 1, None) == _lib.SMK_ERR_INVALID
    assert "workspace" in L.smk_last_error().decode()
    assert two(one, one, one, one, one, 2, 3, 8, 8, 8, 9, None, 0, None) == _lib.SMK_ERR_INVALID
    assert two(one, one, one, one, one + 4, 2, 3, 8, 8, 8, 9, one, 1 << 20, None) == _lib.SMK_ERR_INVALID          # norms: 8 bytes
    assert two(one, one, one, one, one, 2, 3, 8, 8, 8, 9, one + 4, 1 << 20, None) == _lib.SMK_ERR_INVALID          # workspace: 8 bytes
    assert "8-byte" in L.smk_last_error().decode()
    assert two(one, None, one, one, one, 2, 3, 8, 8, 8, 9, one, 1 << 20, None) == _lib.SMK_ERR_INVALID
    assert three(one, one, one, one, one, one, 2, 9, 8, 8, 8, 8, 9, one, 1 << 30, None) == _lib.SMK_ERR_INVALID
    assert "T <= 8" in L.smk_last_error().decode()
    assert three(one, one, one, one, one, one, 2, 3, 8, 8, 8, 8, 9, one, L.smk_tangent3d_orthonormalize_workspace(2, 3, 8, 8, 8) - 1,
                 None) == _lib.SMK_ERR_INVALID
    assert "workspace" in L.smk_last_error().decode()
    assert three(one, one, None, one, one, one, 2, 3, 8, 8, 8, 8, 9, one, 1 << 20, None) == _lib.SMK_ERR_INVALID


def test_kaplan_yorke_dimension_and_ks_entropy_on_hand_made_spectra():
    # the Lorenz attractor's textbook spectrum
    D, truncated = kaplan_yorke_dimension(torch.tensor([0.9, 0.0, -14.57], dtype=torch.float64))
    assert D.dtype == torch.float64 and D.dim() == 0 and abs(float(D) - (2 + 0.9 / 14.57)) <= 1e-15 and not bool(truncated)
    assert abs(float(ks_entropy(torch.tensor([0.9, 0.0, -14.57], dtype=torch.float64))) - 0.9) <= 1e-15
    # all negative: a fixed point
    D, truncated = kaplan_yorke_dimension(torch.tensor([-0.5, -1.0, -3.0], dtype=torch.float64))
    assert float(D) == 0.0 and not bool(truncated) and float(ks_entropy(torch.tensor([-0.5, -1.0, -3.0]))) == 0.0
    # no crossing within k: a lower bound, and it says so
    D, truncated = kaplan_yorke_dimension(torch.tensor([1.0, 0.5], dtype=torch.float64))
    assert float(D) == 2.0 and bool(truncated) and float(ks_entropy(torch.tensor([1.0, 0.5], dtype=torch.float64))) == 1.5
    # unsorted input is sorted first
    D, truncated = kaplan_yorke_dimension(torch.tensor([-14.57, 0.9, 0.0], dtype=torch.float64))
    assert float(D) == float(kaplan_yorke_dimension(torch.tensor([0.9, 0.0, -14.57], dtype=torch.float64))[0]) and not bool(truncated)
    # a crossing after the first exponent; a sum that is exactly zero counts as not yet negative
    D, _ = kaplan_yorke_dimension(torch.tensor([1.0, -4.0, -5.0], dtype=torch.float64))
    assert float(D) == 1.25
    D, truncated = kaplan_yorke_dimension(torch.tensor([1.0, -1.0, -2.0], dtype=torch.float64))
    assert float(D) == 2.0 and not bool(truncated)
    # batched, any leading shape
    spectra = torch.tensor([[0.9, 0.0, -14.57], [-0.5, -1.0, -3.0], [1.0, 0.5, 0.25], [0.0, -14.57, 0.9]], dtype=torch.float64)
    D, truncated = kaplan_yorke_dimension(spectra)
    assert tuple(D.shape) == (4,) and truncated.dtype == torch.bool
    assert torch.allclose(D, torch.tensor([2 + 0.9 / 14.57, 0.0, 3.0, 2 + 0.9 / 14.57], dtype=torch.float64), rtol=0, atol=1e-15)
    assert truncated.tolist() == [False, False, True, False]
    assert torch.allclose(ks_entropy(spectra), torch.tensor([0.9, 0.0, 1.75, 0.9], dtype=torch.float64), rtol=0, atol=1e-15)
    D, truncated = kaplan_yorke_dimension(spectra.view(2, 2, 3))
    assert tuple(D.shape) == (2, 2) and tuple(truncated.shape) == (2, 2) and tuple(ks_entropy(spectra.view(2, 2, 3)).shape) == (2, 2)
    D, _ = kaplan_yorke_dimension(torch.tensor([0.9, float("nan"), -1.0]))
    assert float(D) != float(D)


def test_the_gram_schmidt_keyword_is_checked():
    state = O.draw_state((5, 7), 6.0)
    with pytest.raises(ValueError, match="gram_schmidt='hip' goes with route='hip'"):
        lyapunov_exponents(*state, 4, k=2, gram_schmidt="hip", route="torch")
    with pytest.raises(ValueError, match="gram_schmidt is"):
        lyapunov_exponents(*state, 4, k=2, gram_schmidt="qr", route="torch")
    with pytest.raises(ValueError, match="gram_schmidt is"):
        flow_chaos(*state, 4, gram_schmidt="eager", route="torch")
    with pytest.raises(ValueError, match="gram_schmidt='hip' goes with route='hip'"):
        flow_chaos(*state, 4, gram_schmidt="hip", route="torch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow_chaos(*state, 4)                                        # route="hip" on CPU tensors
    u, v, p, d = (torch.zeros(1, 4, 5 + 1, 6), torch.zeros(1, 4, 5, 6 + 1), torch.zeros(1, 4, 5, 6), torch.zeros(1, 4, 5, 6))
    w = torch.zeros(1, 4 + 1, 5, 6)
    with pytest.raises(ValueError, match="gram_schmidt='hip' goes with route='hip'"):
        lyapunov_exponents3d(u, v, w, p, d, 2, k=2, gram_schmidt="hip", route="torch")
    with pytest.raises(ValueError, match="gram_schmidt is"):
        flow_chaos3d(u, v, w, p, d, 2, gram_schmidt="qr", route="torch")


def test_flow_chaos_on_the_torch_route_is_the_spectrum_plus_the_formulas():
    state = O.draw_state((16, 16), 60.0)
    want = lyapunov_exponents(*state, 4, k=4, route="torch", renorm_every=2, seed=3)
    got = flow_chaos(*state, 4, route="torch", renorm_every=2, seed=3)
    assert isinstance(got, FlowChaos)
    assert torch.equal(got.log_growth, want.log_growth) and tuple(got.exponents.shape) == (O.B, 4) and got.exponents.dtype == torch.float64
    assert torch.equal(got.exponents, want.exponents.sort(dim=1, descending=True).values)
    assert torch.equal(got.lyapunov, got.exponents[:, 0])
    ky, truncated = kaplan_yorke_dimension(want.exponents)
    assert torch.equal(got.kaplan_yorke, ky) and torch.equal(got.truncated, truncated) and got.truncated.dtype == torch.bool
    assert torch.equal(got.ks_entropy, ks_entropy(want.exponents))
    for b in range(O.B):                                             # the formulas once more, written out in Python floats
        lam = sorted(want.exponents[b].tolist(), reverse=True)
        sums = [sum(lam[:j + 1]) for j in range(4)]
        j = sum(s >= 0 for s in sums)
        D = 0.0 if j == 0 else 4.0 if j == 4 else j + sums[j - 1] / abs(lam[j])
        assert abs(float(got.kaplan_yorke[b]) - D) <= 1e-12 and bool(got.truncated[b]) == (j == 4)
        assert abs(float(got.ks_entropy[b]) - sum(max(x, 0.0) for x in lam)) <= 1e-12
    one = flow_chaos(*[s[0] for s in state], 4, route="torch", renorm_every=2, seed=3)          # un-batched: without the B
    assert tuple(one.exponents.shape) == (4,) and one.lyapunov.dim() == 0 and one.kaplan_yorke.dim() == 0 and one.truncated.dim() == 0
