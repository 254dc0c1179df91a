"""CPU-side checks of the tangent-linear 2-D fluid step (smokephysai_amd/physics/fluid_tangent.py): the symbols are
declared, exported and bound; bad arguments are refused; the rule's JVP (torch.autograd.forward_ad over fluid_step_rule) is linear in the
tangent and is the transpose of autograd's VJP along recorded branches in fp64; lyapunov_exponents(route="torch") does not depend on the
norm of tangent0; Gram-Schmidt returns orthonormal tangents."""
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
from smokephysai_amd.physics import (Branches, LyapunovResult, fluid_step_jvp, fluid_step_jvp_rule, fluid_step_rule,   # noqa: E402
                                     fluid_tangent_rollout, lyapunov_exponents)

NEW = ("smk_advect_tangent", "smk_tangent_renorm", "smk_tangent_renorm_workspace")


def _tangents(state, seed, T=None, dtype=torch.float32):
    g = O._gen(seed, *state[3].shape)
    return [torch.randn(s.shape if T is None else (s.shape[0], T) + tuple(s.shape[1:]), generator=g).to(dtype) for s in state]


def _dot(a, b):
    return sum(float((x.double() * y.double()).sum()) for x, y in zip(a, b))


def test_the_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/smokehip.h"
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert len(_lib._SIGNATURES["smk_advect_tangent"]) == 16 and len(_lib._SIGNATURES["smk_tangent_renorm"]) == 14
    assert L.smk_tangent_renorm_workspace.restype is _lib.C.c_int64
    import smokephysai_amd.physics as physics
    for name in ("fluid_step_jvp", "fluid_step_jvp_rule", "fluid_tangent_rollout", "lyapunov_exponents", "LyapunovResult"):
        assert name in physics.__all__ and hasattr(physics, name)
    assert hasattr(physics.SmokeSimulator, "flow_lyapunov")


def test_the_workspace_query_refuses_what_the_entry_points_refuse():
    L = _lib.load()
    assert L.smk_tangent_renorm_workspace(2, 3, 33, 40) > 0 and L.smk_tangent_renorm_workspace(2, 3, 33, 40) % 8 == 0
    assert L.smk_tangent_renorm_workspace(65535, 1, 3, 3) > 0
    for B, T, H, W in ((0, 1, 8, 8), (1, 0, 8, 8), (2, 32768, 8, 8), (65535, 2, 8, 8), (1, 1, 2, 8), (1, 1, 8, 2), (1, 1, 32767, 8), (1, 1, 8, 32767)):
        assert L.smk_tangent_renorm_workspace(B, T, H, W) == -1, (B, T, H, W)


def test_the_entry_points_refuse_bad_shapes_before_touching_anything():
    L = _lib.load()
    one = 4096                   # never dereferenced: every call below is refused on its arguments
    ptr = [one] * 7
    for B, T, H, W, pc, pv, which in ((2, 1, 8, 8, 8, 9, 3), (2, 1, 8, 8, 8, 9, -1), (0, 1, 8, 8, 8, 9, 0), (2, 0, 8, 8, 8, 9, 0),
                                      (3, 32768, 8, 8, 8, 9, 0), (2, 1, 2, 8, 8, 9, 0), (2, 1, 8, 8, 7, 9, 0), (2, 1, 8, 8, 8, 8, 0)):
        assert L.smk_advect_tangent(which, *ptr, B, T, H, W, pc, pv, 0.01, None) == _lib.SMK_ERR_INVALID, (B, T, H, W, pc, pv, which)
    assert L.smk_advect_tangent(0, *([one] * 6), None, 2, 1, 8, 8, 8, 9, 0.01, None) == _lib.SMK_ERR_INVALID
    assert L.smk_advect_tangent(0, one, one, one, one, one, one, one, 2, 1, 8, 8, 8, 9, 0.01, None) == _lib.SMK_ERR_INVALID      # tout aliases
    assert "alias" in L.smk_last_error().decode()
    assert L.smk_tangent_renorm(one, one, one, one, one, 70000, 1, 8, 8, 8, 9, one, 1 << 30, None) == _lib.SMK_ERR_INVALID
    assert L.smk_tangent_renorm(one, one, one, one, one, 2, 1, 8, 8, 8, 9, one, 7, None) == _lib.SMK_ERR_INVALID
    assert "workspace" in L.smk_last_error().decode()
    assert L.smk_tangent_renorm(one, one, one, one, one, 2, 1, 8, 8, 8, 9, None, 0, None) == _lib.SMK_ERR_INVALID
    assert L.smk_tangent_renorm(one, one, one, one, one + 4, 2, 1, 8, 8, 8, 9, one, 1 << 20, None) == _lib.SMK_ERR_INVALID    # norms: 8 bytes


def test_python_refuses_bad_arguments():
    state = O.draw_state((5, 7), 6.0)
    tan = _tangents(state, 1)
    with pytest.raises(ValueError, match="route"):
        fluid_step_jvp(state, tan, route="cuda")
    with pytest.raises(ValueError, match="route"):
        lyapunov_exponents(*state, 4, route="eager")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fluid_step_jvp(state, tan)                                   # route="hip" on CPU tensors
    with pytest.raises(ValueError, match="tangent of v"):
        fluid_step_jvp(state, [tan[0], tan[0], tan[2], tan[3]], route="torch")
    with pytest.raises(ValueError, match="state-shaped"):
        fluid_step_jvp(state, [tan[0][:, None], tan[1], tan[2], tan[3]], route="torch")
    with pytest.raises(ValueError, match="tangents are"):
        fluid_step_jvp(state, tan[:3], route="torch")
    with pytest.raises(ValueError, match="must be"):
        fluid_step_jvp((state[0], state[1], state[2][:, :-1], state[3]), tan, route="torch")
    with pytest.raises(ValueError, match="k <= 8"):
        lyapunov_exponents(*state, 4, k=9, route="torch")
    with pytest.raises(ValueError, match="k <= 8"):
        lyapunov_exponents(*state, 4, k=0, route="torch")
    with pytest.raises(ValueError, match="multiple"):
        lyapunov_exponents(*state, 5, renorm_every=2, route="torch")
    with pytest.raises(ValueError, match="k = 2"):
        lyapunov_exponents(*state, 4, k=2, tangent0=tan, route="torch")
    with pytest.raises(ValueError, match="n_steps"):
        fluid_tangent_rollout(state, tan, 0, route="torch")
    big = [torch.zeros(1).expand(40000, *s.shape[1:]) for s in state]          # B * T = 80000 > 65535, no memory behind it
    with pytest.raises(ValueError, match="exceeds 65535"):
        fluid_step_jvp(big, [t[:, None].expand(40000, 2, *t.shape[1:]) for t in big], route="torch")


@pytest.mark.parametrize("shape", [(3, 3), (5, 7), (33, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_jvp_and_vjp_of_the_rule_are_transposes_in_fp64(shape):
    """<J t, g> = <t, J^T g> along the branches recorded by the fp32 run: forward_ad against autograd, to 1e-12 relative."""
    for dt, amp, J in O.REGIMES:
        state = O.draw_state(shape, amp)
        rec = Branches()
        fluid_step_rule(*state, dt=dt, jacobi_iters=J, branches=rec)
        s64 = [s.double() for s in state]
        t64, g64 = _tangents(state, 11, dtype=torch.float64), _tangents(state, 12, dtype=torch.float64)
        _, jt = fluid_step_jvp_rule(s64, t64, dt=dt, jacobi_iters=J, branches=rec.replayer())
        xs = [s.clone().requires_grad_(True) for s in s64]
        outs = fluid_step_rule(*xs, dt=dt, jacobi_iters=J, branches=rec.replayer())
        jtg = torch.autograd.grad(outs, xs, g64)
        lhs, rhs = _dot(jt, g64), _dot(t64, jtg)
        rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print(f"{shape} dt={dt}: <Jt, g> = {lhs:.15e}, <t, JTg> = {rhs:.15e}, relative mismatch {rel:.2e}")
        assert rel <= 1e-12


def test_the_rules_jvp_is_linear_in_the_tangent():
    state = [s.double() for s in O.draw_state((5, 7), 60.0)]
    a, b = _tangents(state, 21, dtype=torch.float64), _tangents(state, 22, dtype=torch.float64)
    new_a, ja = fluid_step_jvp_rule(state, a)
    _, jb = fluid_step_jvp_rule(state, b)
    _, jc = fluid_step_jvp_rule(state, [2.5 * x - 0.75 * y for x, y in zip(a, b)])
    for name, x, y, z in zip("uvpd", ja, jb, jc):
        assert O.metric(z, 2.5 * x - 0.75 * y) <= 1e-13, name
    want = fluid_step_rule(*state)
    for x, y in zip(new_a, want):
        assert torch.equal(x, y)                                     # the primal is the rule's step
    # [B, T, ...]: tangent i of a T = 3 call is its own call, and the state comes back un-expanded
    stacked = [torch.stack([x, y, x + y], dim=1) for x, y in zip(a, b)]
    new_s, js = fluid_step_jvp_rule(state, stacked)
    for x, y, s, n, w in zip(ja, jb, js, new_s, want):
        assert torch.equal(s[:, 0], x) and torch.equal(s[:, 1], y) and torch.equal(n, w)


def test_lyapunov_exponents_do_not_depend_on_the_norm_of_tangent0():
    state = [s.double() for s in O.simulated_state(steps=10)]
    t0 = _tangents(state, 31, dtype=torch.float64)
    one = lyapunov_exponents(*state, 6, tangent0=t0, route="torch", renorm_every=2)
    assert isinstance(one, LyapunovResult)
    assert tuple(one.exponents.shape) == (O.B, 1) and tuple(one.log_growth.shape) == (O.B, 3, 1) and one.exponents.dtype == torch.float64
    assert torch.allclose(one.exponents, one.log_growth.sum(dim=1) / (6 * 0.01), rtol=0, atol=0)
    pow2 = lyapunov_exponents(*state, 6, tangent0=[1024.0 * t for t in t0], route="torch", renorm_every=2)
    assert torch.equal(pow2.log_growth, one.log_growth)              # a power of two scales every operation exactly
    odd = lyapunov_exponents(*state, 6, tangent0=[1e-3 * t for t in t0], route="torch", renorm_every=2)
    assert float((odd.log_growth - one.log_growth).abs().max()) <= 1e-12
    seeded = lyapunov_exponents(*state, 6, seed=5, route="torch"), lyapunov_exponents(*state, 6, seed=5, route="torch")
    assert torch.equal(seeded[0].log_growth, seeded[1].log_growth)
    final = state
    for _ in range(6):
        final = fluid_step_rule(*final)
    for x, y in zip(one.state, final):
        assert torch.equal(x, y)


def test_gram_schmidt_returns_orthonormal_tangents():
    state = [s.double() for s in O.draw_state((16, 24), 60.0)]
    res = lyapunov_exponents(*state, 3, k=2, route="torch")
    assert tuple(res.exponents.shape) == (O.B, 2) and tuple(res.log_growth.shape) == (O.B, 3, 2)
    assert all(tuple(t.shape) == (O.B, 2) + tuple(s.shape[1:]) for t, s in zip(res.tangents, state))
    for b in range(O.B):
        q = [[t[b, j] for t in res.tangents] for j in range(2)]
        gram = torch.tensor([[_dot(q[i], q[j]) for j in range(2)] for i in range(2)], dtype=torch.float64)
        assert float((gram - torch.eye(2, dtype=torch.float64)).abs().max()) <= 1e-12, gram
    k1 = lyapunov_exponents(*state, 3, k=1, route="torch", tangent0=[t[:, :1] for t in _tangents(state, 0, T=2, dtype=torch.float64)])
    k2 = lyapunov_exponents(*state, 3, k=2, route="torch", tangent0=_tangents(state, 0, T=2, dtype=torch.float64))
    assert float((k1.log_growth[..., 0] - k2.log_growth[..., 0]).abs().max()) <= 1e-12      # the first vector never sees the second
