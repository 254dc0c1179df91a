"""CPU-side checks of the tangent-linear 3-D fluid step (smokephysai_amd/physics/fluid_tangent3d.py), the twin of
tests/test_fluid_tangent_host.py: the symbols are declared, exported and bound; both entry points and the workspace query refuse bad
shapes, null pointers and aliasing before touching anything; Python refuses bad arguments; the rule's JVP (torch.autograd.forward_ad over
fluid_step3d_rule) is linear in the tangent, a [B, T] call equals T single calls, and it is the transpose of autograd's VJP along recorded
branches in fp64; lyapunov_exponents3d(route="torch") does not depend on the norm of tangent0; Gram-Schmidt returns orthonormal
tangents."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step_grad_oracle as O2                                                                     # noqa: E402
import step3d_grad_oracle as O3                                                                   # noqa: E402
import step3d_tangent_oracle as OT                                                                # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd.physics import (Branches, LyapunovResult, fluid_step3d_jvp, fluid_step3d_jvp_rule, fluid_step3d_rule,   # noqa: E402
                                     fluid_tangent_rollout3d, lyapunov_exponents3d)

NEW = ("smk_advect3d_tangent", "smk_tangent3d_renorm", "smk_tangent3d_renorm_workspace")
SHAPES = [(3, 3, 3), (4, 5, 7), (9, 19, 37)]
_sid = lambda s: "x".join(str(n) for n in s)                                                      # noqa: E731


def test_the_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", header).group(1)) == 17           # additive: the version stays
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/smokehip.h"
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert len(_lib._SIGNATURES["smk_advect3d_tangent"]) == 19 and len(_lib._SIGNATURES["smk_tangent3d_renorm"]) == 16
    assert L.smk_tangent3d_renorm_workspace.restype is _lib.C.c_int64
    import smokephysai_amd.physics as physics
    for name in ("fluid_step3d_jvp", "fluid_step3d_jvp_rule", "fluid_tangent_rollout3d", "lyapunov_exponents3d"):
        assert name in physics.__all__ and hasattr(physics, name)
    assert hasattr(physics.SmokeSimulator3D, "flow_lyapunov")


def test_the_workspace_query_refuses_what_the_entry_points_refuse():
    L = _lib.load()
    q = L.smk_tangent3d_renorm_workspace
    assert q(2, 3, 12, 33, 40) > 0 and q(2, 3, 12, 33, 40) % 8 == 0
    assert q(16383, 1, 3, 3, 3) > 0 and q(1, 16383, 3, 3, 3) > 0                                  # B * T * (D + 1) = 65532
    for B, T, D, H, W in ((0, 1, 8, 8, 8), (1, 0, 8, 8, 8), (16384, 1, 3, 8, 8), (2, 8192, 3, 8, 8), (128, 8, 63, 8, 8), (1, 1, 2, 8, 8),
                          (1, 1, 8, 2, 8), (1, 1, 8, 8, 2), (1, 1, 32767, 8, 8), (1, 1, 8, 32767, 8), (1, 1, 8, 8, 32767),
                          (1, 1, 2048, 2048, 2048)):
        assert q(B, T, D, H, W) == -1, (B, T, D, H, W)


def test_the_entry_points_refuse_bad_shapes_before_touching_anything():
    L = _lib.load()
    one = 4096                   # never dereferenced: every call below is refused on its arguments
    ptr = [one] * 9
    for B, T, D, H, W, pc, pv, which in ((2, 1, 8, 8, 8, 8, 9, 4), (2, 1, 8, 8, 8, 8, 9, -1), (0, 1, 8, 8, 8, 8, 9, 0), (2, 0, 8, 8, 8, 8, 9, 0),
                                         (3, 4096, 8, 8, 8, 8, 9, 0), (2, 1, 2, 8, 8, 8, 9, 0), (2, 1, 8, 2, 8, 8, 9, 0),
                                         (2, 1, 8, 8, 8, 7, 9, 0), (2, 1, 8, 8, 8, 8, 8, 0)):
        assert L.smk_advect3d_tangent(which, *ptr, B, T, D, H, W, pc, pv, 0.01, None) == _lib.SMK_ERR_INVALID, (B, T, D, H, W, pc, pv, which)
    good = (2, 1, 8, 8, 8, 8, 9)
    for hole in range(9):                                            # each pointer null in turn
        args = [one + 64 * i for i in range(9)]
        args[hole] = None
        assert L.smk_advect3d_tangent(0, *args, *good, 0.01, None) == _lib.SMK_ERR_INVALID, hole
        assert "null" in L.smk_last_error().decode()
    for twin in range(8):                                            # tout the same buffer as each input in turn
        args = [one + 64 * i for i in range(9)]
        args[twin] = args[8]
        assert L.smk_advect3d_tangent(0, *args, *good, 0.01, None) == _lib.SMK_ERR_INVALID, twin
        assert "alias" in L.smk_last_error().decode()
    f = [one + 64 * i for i in range(5)]
    assert L.smk_tangent3d_renorm(*f, one, 70000, 1, 8, 8, 8, 8, 9, one, 1 << 30, None) == _lib.SMK_ERR_INVALID
    assert L.smk_tangent3d_renorm(*f, one, 2, 1, 8, 8, 8, 8, 9, one, 7, None) == _lib.SMK_ERR_INVALID
    assert "workspace" in L.smk_last_error().decode()
    assert L.smk_tangent3d_renorm(*f, one, 2, 1, 8, 8, 8, 8, 9, None, 0, None) == _lib.SMK_ERR_INVALID
    assert L.smk_tangent3d_renorm(*f, one + 4, 2, 1, 8, 8, 8, 8, 9, one, 1 << 20, None) == _lib.SMK_ERR_INVALID       # norms: 8 bytes
    assert L.smk_tangent3d_renorm(*f, one, 2, 1, 8, 8, 8, 8, 9, one + 4, 1 << 20, None) == _lib.SMK_ERR_INVALID       # workspace: 8 bytes
    for hole in range(6):
        args = f + [one]
        args[hole] = None
        assert L.smk_tangent3d_renorm(*args, 2, 1, 8, 8, 8, 8, 9, one, 1 << 20, None) == _lib.SMK_ERR_INVALID, hole


def test_python_refuses_bad_arguments():
    state = O3.draw_state3d((4, 5, 7), 5.0)
    tan = OT.tangents(state, 1)
    with pytest.raises(ValueError, match="fluid_step3d_jvp: route"):
        fluid_step3d_jvp(state, tan, route="cuda")
    with pytest.raises(ValueError, match="lyapunov_exponents3d: route"):
        lyapunov_exponents3d(*state, 4, route="eager")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fluid_step3d_jvp(state, tan)                                 # route="hip" on CPU tensors
    with pytest.raises(ValueError, match="tangent of v"):
        fluid_step3d_jvp(state, [tan[0], tan[0], tan[2], tan[3], tan[4]], route="torch")
    with pytest.raises(ValueError, match="tangent of w"):
        fluid_step3d_jvp(state, [tan[0], tan[1], tan[3], tan[3], tan[4]], route="torch")
    with pytest.raises(ValueError, match="state-shaped"):
        fluid_step3d_jvp(state, [tan[0][:, None], *tan[1:]], route="torch")
    with pytest.raises(ValueError, match=r"tangents are \(tu, tv, tw, tp, tdensity\)"):
        fluid_step3d_jvp(state, tan[:4], route="torch")
    with pytest.raises(ValueError, match="must be"):
        fluid_step3d_jvp((*state[:3], state[3][:, :-1], state[4]), tan, route="torch")
    with pytest.raises(ValueError, match="k <= 8"):
        lyapunov_exponents3d(*state, 4, k=9, route="torch")
    with pytest.raises(ValueError, match="k <= 8"):
        lyapunov_exponents3d(*state, 4, k=0, route="torch")
    with pytest.raises(ValueError, match="multiple"):
        lyapunov_exponents3d(*state, 5, renorm_every=2, route="torch")
    with pytest.raises(ValueError, match="k = 2"):
        lyapunov_exponents3d(*state, 4, k=2, tangent0=tan, route="torch")
    with pytest.raises(ValueError, match="branches"):
        lyapunov_exponents3d(*state, 4, branches=Branches())
    with pytest.raises(ValueError, match="n_steps"):
        fluid_tangent_rollout3d(state, tan, 0, route="torch")
    big = [torch.zeros(1).expand(4000, *s.shape[1:]) for s in state]           # B * T * (D + 1) = 80000 > 65535, no memory behind it
    with pytest.raises(ValueError, match=r"B \* T \* \(D \+ 1\) = 80000 exceeds 65535"):
        fluid_step3d_jvp(big, [t[:, None].expand(4000, 4, *t.shape[1:]) for t in big], route="torch")


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_jvp_and_vjp_of_the_rule_are_transposes_in_fp64(shape):
    """<J t, g> = <t, J^T g> along the branches recorded by the fp32 run: forward_ad against autograd, to 1e-12 relative."""
    for dt, amp, J in O3.REGIMES:
        state = O3.draw_state3d(shape, amp)
        rec = Branches()
        fluid_step3d_rule(*state, dt=dt, jacobi_iters=J, branches=rec)
        s64 = [s.double() for s in state]
        t64, g64 = OT.tangents(state, 11, dtype=torch.float64), OT.tangents(state, 12, dtype=torch.float64)
        _, jt = fluid_step3d_jvp_rule(s64, t64, dt=dt, jacobi_iters=J, branches=rec.replayer())
        xs = [s.clone().requires_grad_(True) for s in s64]
        outs = fluid_step3d_rule(*xs, dt=dt, jacobi_iters=J, branches=rec.replayer())
        jtg = torch.autograd.grad(outs, xs, g64)
        lhs, rhs = OT.dot(jt, g64), OT.dot(t64, jtg)
        rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print(f"{shape} dt={dt}: <Jt, g> = {lhs:.15e}, <t, JTg> = {rhs:.15e}, relative mismatch {rel:.2e}")
        assert rel <= 1e-12


def test_the_rules_jvp_is_linear_in_the_tangent_and_a_T_call_is_T_single_calls():
    state = [s.double() for s in O3.draw_state3d((4, 5, 7), 50.0)]
    a, b = OT.tangents(state, 21, dtype=torch.float64), OT.tangents(state, 22, dtype=torch.float64)
    new_a, ja = fluid_step3d_jvp_rule(state, a)
    _, jb = fluid_step3d_jvp_rule(state, b)
    _, jc = fluid_step3d_jvp_rule(state, [2.5 * x - 0.75 * y for x, y in zip(a, b)])
    for name, x, y, z in zip(OT.NAMES, ja, jb, jc):
        assert O2.metric(z, 2.5 * x - 0.75 * y) <= 1e-13, name
    want = fluid_step3d_rule(*state)
    for x, y in zip(new_a, want):
        assert torch.equal(x, y)                                     # the primal is the rule's step
    # [B, T, ...]: tangent i of a T = 3 call is its own call, and the state comes back un-expanded
    stacked = [torch.stack([x, y, x + y], dim=1) for x, y in zip(a, b)]
    new_s, js = fluid_step3d_jvp_rule(state, stacked)
    for x, y, s, n, w in zip(ja, jb, js, new_s, want):
        assert torch.equal(s[:, 0], x) and torch.equal(s[:, 1], y) and torch.equal(n, w)
    # un-batched: the leading dimension comes and goes
    new_1, j1 = fluid_step3d_jvp_rule([s[0] for s in state], [t[0] for t in a])
    for x, y, n, w in zip(j1, ja, new_1, want):
        assert torch.equal(x, y[0]) and torch.equal(n, w[0])


def test_lyapunov_exponents_do_not_depend_on_the_norm_of_tangent0():
    state = [s.double() for s in OT.lyapunov_state(False)]
    t0 = OT.tangents(state, 31, dtype=torch.float64)
    one = lyapunov_exponents3d(*state, 6, tangent0=t0, route="torch", renorm_every=2)
    assert isinstance(one, LyapunovResult)
    assert tuple(one.exponents.shape) == (OT.B, 1) and tuple(one.log_growth.shape) == (OT.B, 3, 1) and one.exponents.dtype == torch.float64
    assert torch.allclose(one.exponents, one.log_growth.sum(dim=1) / (6 * 0.01), rtol=0, atol=0)
    pow2 = lyapunov_exponents3d(*state, 6, tangent0=[1024.0 * t for t in t0], route="torch", renorm_every=2)
    assert torch.equal(pow2.log_growth, one.log_growth)              # a power of two scales every operation exactly
    odd = lyapunov_exponents3d(*state, 6, tangent0=[1e-3 * t for t in t0], route="torch", renorm_every=2)
    assert float((odd.log_growth - one.log_growth).abs().max()) <= 1e-12
    seeded = lyapunov_exponents3d(*state, 6, seed=5, route="torch"), lyapunov_exponents3d(*state, 6, seed=5, route="torch")
    assert torch.equal(seeded[0].log_growth, seeded[1].log_growth)
    final = state
    for _ in range(6):
        final = fluid_step3d_rule(*final)
    assert len(one.state) == 5
    for x, y in zip(one.state, final):
        assert torch.equal(x, y)


def test_gram_schmidt_returns_orthonormal_tangents():
    state = [s.double() for s in O3.draw_state3d((4, 5, 7), 50.0)]
    res = lyapunov_exponents3d(*state, 3, k=2, route="torch")
    assert tuple(res.exponents.shape) == (OT.B, 2) and tuple(res.log_growth.shape) == (OT.B, 3, 2)
    assert len(res.tangents) == 5 and all(tuple(t.shape) == (OT.B, 2) + tuple(s.shape[1:]) for t, s in zip(res.tangents, state))
    for b in range(OT.B):
        q = [[t[b, j] for t in res.tangents] for j in range(2)]
        gram = torch.tensor([[OT.dot(q[i], q[j]) for j in range(2)] for i in range(2)], dtype=torch.float64)
        assert float((gram - torch.eye(2, dtype=torch.float64)).abs().max()) <= 1e-12, gram
    k1 = lyapunov_exponents3d(*state, 3, k=1, route="torch", tangent0=[t[:, :1] for t in OT.tangents(state, 0, T=2, dtype=torch.float64)])
    k2 = lyapunov_exponents3d(*state, 3, k=2, route="torch", tangent0=OT.tangents(state, 0, T=2, dtype=torch.float64))
    assert float((k1.log_growth[..., 0] - k2.log_growth[..., 0]).abs().max()) <= 1e-12      # the first vector never sees the second
