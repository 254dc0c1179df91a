"""Child process of tests/test_jacobi_fused_sweep.py (SMK_JACOBI_PERSIST is read once per process): runs every case on the GPU, compares
word for word with the CPU oracle here, and prints one line `RESULT <json>`.  Run alone it prints the same line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle                                                            # noqa: E402
from smokephysai_amd.physics import NavierStokesSimulator               # noqa: E402

KEYS = ("u", "v", "p", "density")
# (H, W, batch): one, two and four cells per lane; the last has more bands x grids than one persistent launch holds
SHAPES = [(64, 64, 3), (128, 128, 3), (256, 256, 3), (320, 64, 100)]
J = 40
LO, HI = np.float32(2.0 ** -100), np.float32(2.0 ** 100)


def differing_words(got, want):
    """cells whose 32-bit words differ; two NaNs count as equal whatever their payload"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return int((~same).sum())


def guard(d):
    a = np.abs(d)
    return (a == 0) | ((a >= LO) & (a <= HI))                           # (NaN and Inf compare False)


def tiles(H, plan):
    """[r0, r1) of the rows each band of a grid holds in registers, owned and halo rows alike (k_jacobi_band's own arithmetic)"""
    nb, TR, halo = plan["bands_per_grid"], plan["rows_per_workgroup"], plan["halo_rows"]
    out = []
    for band in range(nb):
        own0 = 0 if band == 0 else (TR - halo) + (band - 1) * (TR - 2 * halo)
        r0 = 0 if band == 0 else (H - TR if band == nb - 1 else own0 - halo)
        r0 = max(0, min(r0, H - TR))
        out.append((r0, r0 + TR))
    return out


def step_divergence(o):
    """the divergence the projection of o's NEXT step sweeps on: buoyancy, the two velocity diffusions, navier_stokes.py:136"""
    c = oracle.OracleNS((o.h, o.w), dt=o.dt, viscosity=o.viscosity, jacobi_iters=o.jacobi_iters)
    c.u, c.v, c.density = o.u.copy(), o.v.copy(), o.density.copy()
    c.buoyancy()
    c.u, c.v = c.diffusion_step(c.u, c.viscosity), c.diffusion_step(c.v, c.viscosity)
    return c.divergence()


def expected_forms(div, H, plan):
    """per band: 1 where every divergence value of the rows the band holds passes the guard -- if the step's kernel has two forms at all"""
    if plan.get("cell_forms_of_a_step") != 2:
        return [0] * plan["bands_per_grid"]
    rows = sorted({int(r) for r, _ in np.argwhere(~guard(div))})
    return [0 if any(r0 <= r < r1 for r in rows) else 1 for (r0, r1) in tiles(H, plan)]


def state_mismatch(ns, orcs, grids, keys=KEYS):
    torch.cuda.synchronize()
    bad = {}
    for k in keys:
        got = getattr(ns, k).cpu().numpy()
        n = sum(differing_words(got[b], getattr(orcs[b], k)) for b in grids)
        if n:
            bad[k] = n
    return bad


def dense(H, W, B, vel=40.0, check=None, poison=None):
    """two whole steps from the dense random states of test_hip_physics.test_whole_steps_from_dense_random_states_bit_exact_vs_oracle;
    `check`: the grids compared with the oracle (default all); `poison`: that grid gets one NaN in v and one Inf in u -- then one step,
    and of the poisoned grid the pressure alone is compared: it is final before the advection, whose index arithmetic on NaN coordinates is
    not what this test is about"""
    check = list(range(B)) if check is None else check
    ns = NavierStokesSimulator((H, W), batch_size=B, jacobi_iters=J)
    plan = ns.jacobi_plan()["projection"]
    orcs = []
    for b in range(B):
        rng = np.random.RandomState(1000 * H + W + b)
        o = oracle.OracleNS((H, W), jacobi_iters=J)
        o.u = (rng.standard_normal((H + 1, W)) * vel).astype(np.float32)
        o.v = (rng.standard_normal((H, W + 1)) * vel).astype(np.float32)
        o.p = (rng.standard_normal((H, W)) * 0.1).astype(np.float32)
        o.density = rng.uniform(0.0, 1.8, (H, W)).astype(np.float32)
        if b == poison:
            o.v[5, W - 7] = np.nan
            o.u[H // 2 + 3, W // 3] = np.inf
        orcs.append(o)
    for k in KEYS:
        setattr(ns, k, torch.from_numpy(np.stack([getattr(o, k) for o in orcs])))
    frame = torch.empty(B, H, W, device="cuda")
    steps = []
    clean = [b for b in check if b != poison]
    for _ in range(2 if poison is None else 1):
        expect = {b: expected_forms(step_divergence(orcs[b]), H, plan) for b in check}
        ns.step_into(frame, 1)
        forms = ns.sweep_forms()
        want = {b: orcs[b].step() for b in check}
        bad = state_mismatch(ns, orcs, clean)
        if poison is not None:
            bad.update({"poisoned_" + k: v for k, v in state_mismatch(ns, orcs, [poison], ("p",)).items()})
        n = sum(differing_words(frame[b].cpu().numpy(), want[b]) for b in clean)
        if n:
            bad["frame"] = n
        steps.append({"forms": forms, "expect": expect, "mismatch": bad,
                      "oracle_nan_p": {b: int(np.isnan(orcs[b].p).sum()) for b in check}})
    return {"plan": plan, "tiles": tiles(H, plan), "steps": steps}


def from_rest(N, B, check):
    """one source per grid on a zero state, J = 100, four steps; `check`: the grids compared with the oracle"""
    ns = NavierStokesSimulator((N, N), batch_size=B, jacobi_iters=100)
    rng = np.random.RandomState(N + B)
    srcs = [(b, int(rng.randint(20, N - 20)), int(rng.randint(20, N - 20)), 8, float(rng.uniform(0.5, 2.0))) for b in range(B)]
    ns.add_smoke_sources(srcs)
    torch.cuda.synchronize()
    d0 = ns.density.cpu().numpy()
    orcs = {}
    for b in check:
        orcs[b] = oracle.OracleNS((N, N), jacobi_iters=100)
        orcs[b].density = d0[b].copy()
    frame = torch.empty(B, N, N, device="cuda")
    plan = ns.jacobi_plan()["projection"]
    steps = []
    for t in range(4):
        expect = {b: expected_forms(step_divergence(o), N, plan) for b, o in orcs.items()}
        ns.step_into(frame, 1)
        forms = ns.sweep_forms()
        for o in orcs.values():
            o.step()
        tiny = np.float32(2.0 ** -126)
        denormal = sum(int(((np.abs(o.p) < tiny) & (o.p != 0)).sum()) for o in orcs.values())
        steps.append({"forms": forms, "expect": expect, "mismatch": state_mismatch(ns, orcs, check), "oracle_denormal_p": denormal})
    return {"plan": plan, "tiles": tiles(N, plan), "steps": steps}


CRAFTED_CELL = (128, 85)            # row 128 of a 256-row grid lies in two bands of the 256^2 x 64 plan: rows 54-149 and 108-203


def crafted(kind, check=(0, 1, 63)):
    """One whole step of 64 grids of 256^2 (the plan of the kernel with both cell forms) whose divergence is ordinary everywhere, but for
    one cell of grid 1: `tiny` 2^-120, `bound` exactly 2^-100.  With viscosity 0 and no density the step's buoyancy and diffusion leave
    the velocities as they are (x + 0 * laplacian, v + dt * 0), on the device as in the oracle, so the projection sweeps on exactly the
    divergence of the crafted u, v; dt = 2^-7 makes its division exact."""
    H = W = 256
    B, dt = 64, 2.0 ** -7
    i0, j0 = CRAFTED_CELL
    ns = NavierStokesSimulator((H, W), dt=dt, viscosity=0.0, batch_size=B, jacobi_iters=J)
    plan = ns.jacobi_plan()["projection"]
    orcs = []
    for b in range(B):
        rng = np.random.RandomState(77 * H + W + b)
        o = oracle.OracleNS((H, W), dt=dt, viscosity=0.0, jacobi_iters=J)
        o.u = (np.arange(H + 1, dtype=np.float32)[:, None] * rng.uniform(0.5, 2.0, W).astype(np.float32)[None, :]).astype(np.float32)
        o.v = rng.standard_normal((H, W + 1)).astype(np.float32)
        o.p = (rng.standard_normal((H, W)) * 0.1).astype(np.float32)
        if b == 1:
            o.v[i0, j0] = o.v[i0, j0 + 1] = 0.0
            o.u[i0, j0] = 0.0
            o.u[i0 + 1, j0] = {"tiny": 2.0 ** -127, "bound": 2.0 ** -107}[kind]
        orcs.append(o)
    for k in KEYS:
        setattr(ns, k, torch.from_numpy(np.stack([getattr(o, k) for o in orcs])))
    div = {b: step_divergence(orcs[b]) for b in check}
    untouched = all(differing_words(div[b], orcs[b].divergence()) == 0 for b in check)      # the prologue changes nothing here
    fails = {b: np.argwhere(~guard(div[b])).tolist() for b in check}
    expect = {b: expected_forms(div[b], H, plan) for b in check}
    frame = torch.empty(B, H, W, device="cuda")
    ns.step_into(frame, 1)
    forms = ns.sweep_forms()
    want = {b: orcs[b].step() for b in check}
    bad = state_mismatch(ns, orcs, check)
    n = sum(differing_words(frame[b].cpu().numpy(), want[b]) for b in check)
    if n:
        bad["frame"] = n
    return {"plan": plan, "tiles": tiles(H, plan), "forms": forms, "expect": expect, "mismatch": bad, "guard_fails": fails,
            "cell_div": float(div[1][i0, j0]), "prologue_leaves_divergence": untouched}


def main():
    out = {"persist_env": os.environ.get("SMK_JACOBI_PERSIST"), "dense": {}, "rest": {}, "crafted": {}}
    for (H, W, B) in SHAPES:
        key = "%dx%dxB%d" % (H, W, B)
        out["dense"][key] = dense(H, W, B)
    # the 256^2 x 64 plan: 4 cells per lane, 6 rows per wave, the one kernel with both cell forms
    out["dense"]["256x256xB64"] = dense(256, 256, 64, check=[0, 21, 63])
    out["dense"]["256x256xB64:naninf"] = dense(256, 256, 64, check=[0, 21, 63], poison=21)
    for kind in ("tiny", "bound"):
        out["crafted"][kind] = crafted(kind)
    out["rest"]["128xB3"] = from_rest(128, 3, [0, 1, 2])
    out["rest"]["256xB3"] = from_rest(256, 3, [0, 1, 2])
    out["rest"]["256xB64"] = from_rest(256, 64, [0, 21, 63])
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
