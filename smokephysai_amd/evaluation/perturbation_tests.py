"""Perturbation tests -- drop-in for src/evaluation/perturbation_tests.py (PerturbationTester).

Same methods, arguments, defaults and result keys; the work underneath is batched:
  physics_perturbation_test: every scenario is drawn first (the same np.random calls in the same order as the reference's loop;
      simulation draws nothing), then all scenarios run as the grids of ONE batched SmokeSimulator (bit-identical frames to the
      serial loop) and the num_tests x 20 frames go through the model in chunks of `batch_size`.  The caller's simulator is left
      as the reference's loop leaves it: last scenario's final state, history holding the frames the loop would have appended.
  gaussian_noise_test: every noise tensor is drawn first -- randn_like(test_data) * level, in level order -- then the baseline
      and all noisy copies run as one chunked forward.  The reference interleaves its draws with its forwards (the model's chaos
      term draws from the same torch generator), so a seeded run matches the reference's numbers in distribution, not exactly.
  adversarial_test: the reference's PGD loop, with the gradient taken by torch.autograd.grad with respect to the perturbation
      only, the parameters' requires_grad switched off for the attack (and restored): no weight-gradient GEMMs run and no .grad
      is left on the model's parameters (the reference's loss.backward() accumulates them there).

Volumes.  gaussian_noise_test takes what `model(x)` takes: on a SmokePhysNet3D, volumes [B, 1, D, H, W] run as they are (so does
RobustnessEvaluator.evaluate_reconstruction_quality, given a 2-D target such as the rendered volume).  adversarial_test compares the 2-D
reconstruction with the front view of the clean volume (SPEC_3D.md section 10) and perturbs the volume; with input_grad == "hip" the
gradient reaches the volume through Encoder3D's 'frozen' route (smk_conv3d_s7_dgrad).  With render=RenderSettings(...) the model is an
IMAGE model that is shown the render of the perturbed volume: the perturbation lives on the smoke, the gradient reaches it through the
render's backward (smk_volume_render_backward), and with azimuth=... as well from one or several orbit views of it
(physics.render_orbit(..., differentiable=True), smk_volume_render_orbit_backward), or with elevation=... from pitched views
(physics.render_camera(..., differentiable=True), smk_volume_render_camera_backward).  viewpoint_test shows an IMAGE model the same volumes from a ring of camera azimuths
(physics.render_orbit, SPEC_3D.md section 10 "Orbit views") and reports how far its physics features move with the viewpoint; with
elevation=... the ring is seen from above or below (physics.render_camera, "Free camera").
physics_perturbation_test is 2-D only.
adversarial_test(..., simulate=FluidRollout(steps=k)) perturbs the INITIAL smoke of 2-D frames: the model sees the density after k steps of
the stepper, and the gradient reaches the initial density through physics.fluid_step's adjoint kernels (csrc/fluid_grad.hip).
adversarial_test(..., simulate=FluidRollout3D(steps=k)) does the same for volumes [B, 1, D, H, W] through physics.fluid_step3d
(csrc/fluid_grad3d.hip): alone a volume model sees the evolved volume, with render= (and azimuth= / elevation=) an image model sees its render.
"""
import numbers
import warnings
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..physics import SmokeSimulator


def draw_scenarios(num_tests: int, h: int, w: int) -> List[List[tuple]]:
    """The smoke sources of physics_perturbation_test's scenarios, drawn from the global np.random exactly as the reference's loop
    draws them (perturbation_tests.py:113-118): per test randint(1, 4) sources, each x = randint(20, w-20),
    y = randint(20, h-20), intensity = uniform(0.5, 2.0).  Returns one list of (x, y, intensity) per test."""
    scenarios = []
    for _ in range(num_tests):
        sources = []
        for _ in range(np.random.randint(1, 4)):
            x = np.random.randint(20, w - 20)
            y = np.random.randint(20, h - 20)
            intensity = np.random.uniform(0.5, 2.0)
            sources.append((x, y, intensity))
        scenarios.append(sources)
    return scenarios


def _chunked_forward(model: nn.Module, frames: torch.Tensor, batch_size: int, keys) -> Dict[str, torch.Tensor]:
    """model(frames[i:i+batch_size]) over frames [N, 1, H, W] (no_grad); the outputs named in `keys`, concatenated."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    outs = {k: [] for k in keys}
    with torch.no_grad():
        for s in range(0, frames.shape[0], batch_size):
            pred = model(frames[s:s + batch_size])
            for k in keys:
                outs[k].append(pred[k])
    return {k: torch.cat(v) for k, v in outs.items()}


class PerturbationTester:
    """Perturbation tester (perturbation_tests.py:8-146)."""

    def __init__(self, device: str = 'cuda'):
        self.device = device

    def gaussian_noise_test(self, model: nn.Module, test_data: torch.Tensor,
                            noise_levels: List[float] = [0.01, 0.05, 0.1, 0.2], *, batch_size: int = 64) -> Dict:
        """{'gaussian_<level>': {'feature_stability', 'reconstruction_mse'}} (perturbation_tests.py:14-52).  All noise is drawn
        before any forward, randn_like(test_data) * level in level order; see the module docstring."""
        model.eval()
        noisy = [torch.clamp(test_data + torch.randn_like(test_data) * level, 0, 1) for level in noise_levels]
        B = test_data.shape[0]
        out = _chunked_forward(model, torch.cat([test_data] + noisy), batch_size, ('latent_features', 'reconstructed'))
        base_feat, base_rec = out['latent_features'][:B], out['reconstructed'][:B]
        results = {}
        for i, level in enumerate(noise_levels):
            feat = out['latent_features'][(i + 1) * B:(i + 2) * B]
            rec = out['reconstructed'][(i + 1) * B:(i + 2) * B]
            results[f'gaussian_{level}'] = {
                'feature_stability': F.cosine_similarity(base_feat, feat, dim=1).mean().item(),
                'reconstruction_mse': F.mse_loss(rec, base_rec).item(),
            }
        return results

    def viewpoint_test(self, model: nn.Module, volumes: torch.Tensor, azimuths=tuple(range(0, 360, 30)), *, settings=None,
                       batch_size: int = 64, elevation=None) -> Dict:
        """Does the model's answer depend on where the camera stood?  model: an image model; volumes: [B, 1, D, H, W].  Every volume is
        rendered from every azimuth (degrees) by ONE render_orbit call, and the B x V frames go through the model in chunks of
        `batch_size` (eval, no_grad).  Returns
          'viewpoint_feature_stability': the mean over the further views and the volumes of the cosine similarity between the
              physics_features of that view and of the first view (as gaussian_noise_test forms its feature_stability; 1.0 with one view),
          'viewpoint_feature_variance': the variance of physics_features over the views (population), averaged over volumes and features,
          'per_azimuth': {azimuth in degrees: that view's stability against the first; 1.0 for the first itself},
          'num_views': V.
        elevation: None renders the horizontal ring with render_orbit.  A number of degrees in [-90, 90] renders the same ring of
        azimuths from that elevation (positive: looking down on the smoke) with ONE render_camera call, and the result carries
        'elevation' as well."""
        from ..physics import render_camera, render_orbit
        if volumes.dim() != 5 or volumes.shape[1] != 1:
            raise ValueError(f"viewpoint_test: volumes [B, 1, D, H, W], got {tuple(volumes.shape)}")
        angles = [float(a) for a in azimuths]
        if not angles:
            raise ValueError("viewpoint_test: at least one azimuth")
        model.eval()
        B, V = volumes.shape[0], len(angles)
        if elevation is not None:
            if isinstance(elevation, bool) or not isinstance(elevation, numbers.Real):
                raise ValueError(f"viewpoint_test: elevation is None or a number of degrees, got {elevation!r}")
            elevation = float(elevation)
        with torch.no_grad():
            if elevation is None:
                frames = render_orbit(volumes[:, 0].detach(), angles, settings)              # [B, V, H, W]
            else:
                frames = render_camera(volumes[:, 0].detach(), angles, elevation, settings)  # [B, V, H, W]
        H, W = frames.shape[-2:]
        feats = _chunked_forward(model, frames.view(B * V, 1, H, W), batch_size, ('physics_features',))['physics_features'].view(B, V, -1)
        further = [F.cosine_similarity(feats[:, 0], feats[:, k], dim=1).mean().item() for k in range(1, V)]
        result = {
            'viewpoint_feature_stability': float(np.mean(further)) if further else 1.0,
            'viewpoint_feature_variance': feats.var(dim=1, unbiased=False).mean().item(),
            'per_azimuth': dict(zip(angles, [1.0] + further)),
            'num_views': V,
        }
        if elevation is not None:
            result['elevation'] = elevation
        return result

    def adversarial_test(self, model: nn.Module, test_data: torch.Tensor, epsilon: float = 0.1, num_steps: int = 10, *,
                         target: Optional[torch.Tensor] = None, render=None, azimuth=None, elevation=None, simulate=None) -> Dict:
        """PGD on the reconstruction error (perturbation_tests.py:54-98): {'adversarial_feature_stability',
        'adversarial_perturbation_norm'}.  The gradient is taken with respect to the perturbation only (module docstring): with every
        parameter frozen, a SmokePhysNet with input_grad == "hip" serves 128^2 / 256^2 frames on its libsmokehip route (forward and
        backward; no MIOpen call), a SmokePhysNet3D volumes of the training kernels' shapes, and anything else the PyTorch modules.
        target: the image the reconstruction is compared with in the loss -mse(reconstructed, target).  Default: test_data itself for
        frames [B, 1, H, W] (the reference's line); for volumes [B, 1, D, H, W] the front view of the clean volume,
        render_volumes(test_data[:, 0])[:, None] with the default RenderSettings.  An image of another size than the reconstruction (the
        head always emits 128 x 128) is brought there with F.adaptive_avg_pool2d, as train.py does with its targets.
        render: a RenderSettings; test_data is then volumes [B, 1, D, H, W] and `model` an image model, which sees
        render_volumes(clamp(test_data + delta, 0, 1)[:, 0], render)[:, None] -- which change to the SMOKE changes the model's answer.  The
        perturbation (and its norm) is the volume's; the default comparison image is the render of the clean volume under the same
        settings; the closing forwards run on the rendered frames.  None: the code path without it.
        azimuth (needs render=): a number of degrees or a sequence of V of them.  The model then sees the perturbed volume from where the
        camera stands, render_orbit(clamp(test_data + delta, 0, 1)[:, 0], azimuth, render, differentiable=True) as [B*V, 1, H, W] frames
        (SPEC_3D.md section 10, "Orbit views -- Gradient"; smk_volume_render_orbit_backward): the loss is the mean over all B*V frames,
        the default comparison image the clean volume's render from the same views, and the closing forwards run over the B*V frames.
        None: the front view above.
        elevation (needs render=): a number of degrees in [-90, 90] or a sequence of them.  The views are then the free camera's,
        render_camera(..., azimuth, elevation, render, differentiable=True) (SPEC_3D.md section 10, "Free camera -- Gradient";
        smk_volume_render_camera_backward), azimuth (0 when not given) and elevation paired view by view as render_camera pairs them;
        everything else as with azimuth=.  None: the code path without it.
        simulate: a physics.FluidRollout(steps=k, dt=..., viscosity=..., jacobi_iters=...); test_data is then initial densities
        [B, 1, H, W] at rest (u = v = p = 0) and the model sees the density after k steps of clamp(test_data + delta, 0, 1) -- which change
        to the smoke a frame GREW OUT OF changes the model's answer.  The gradient reaches the initial smoke through the stepper's adjoint
        kernels (physics.fluid_step); the perturbation (and its norm) is the initial smoke's, the default comparison
        image the clean rollout.  Not together with render=.  A grid whose back-traces move a cell or more has no gradient on that route
        (NaN): a non-finite perturbation after the loop raises.  None: the code path without it.
        simulate: a physics.FluidRollout3D(steps=k, ...); test_data is then initial VOLUMES [B, 1, D, H, W] at rest (u = v = w = p = 0) and
        the gradient reaches them through the 3-D stepper's adjoint kernels (physics.fluid_step3d).  Alone, the
        model is a volume model (SmokePhysNet3D) that sees the evolved volume, and the default target is the front view of the clean
        evolved volume (the 5-D rule above).  With render= (and azimuth= / elevation= as above) an image model sees the render of the
        evolved volume; the perturbation (and its norm) is the initial volume's and the default comparison image is the clean rollout's
        render from the same views.  The same one-cell limit and the same RuntimeError hold."""
        model.eval()
        from ..physics.fluid_grad3d import FluidRollout3D
        evolve = None                        # the 3-D rollout in front of whatever the model sees of a volume
        if isinstance(simulate, FluidRollout3D):
            if test_data.dim() != 5 or test_data.shape[1] != 1:
                raise ValueError("adversarial_test: with simulate=FluidRollout3D(...), test_data must be initial volumes [B, 1, D, H, W]")
            test_data = test_data.detach().float().contiguous()
            evolve = lambda v: simulate(v[:, 0])[:, None]                       # noqa: E731
        elif simulate is not None and render is not None:
            raise ValueError("adversarial_test: simulate= and render= are two different ways to what the model sees: give one")
        if azimuth is not None and render is None:
            raise ValueError("adversarial_test: azimuth= needs render=RenderSettings(...): it is the rendered volume that is seen from there")
        if elevation is not None and render is None:
            raise ValueError("adversarial_test: elevation= needs render=RenderSettings(...): it is the rendered volume that is seen from there")
        shown = lambda x: x                  # noqa: E731  what the model sees of the (perturbed) data
        if simulate is not None and evolve is None:
            from ..physics.fluid_grad import FluidRollout
            if not isinstance(simulate, FluidRollout):
                raise TypeError("adversarial_test: simulate must be a physics.FluidRollout or a physics.FluidRollout3D")
            if test_data.dim() != 4 or test_data.shape[1] != 1:
                raise ValueError("adversarial_test: with simulate=, test_data must be initial densities [B, 1, H, W]")
            test_data = test_data.detach().float().contiguous()
            shown = lambda d: simulate(d[:, 0])[:, None]                        # noqa: E731
            if target is None:
                with torch.no_grad():
                    target = shown(test_data)
        elif render is not None:
            from ..physics.render import RenderSettings, render_volumes
            if not isinstance(render, RenderSettings):
                raise TypeError("adversarial_test: render must be a RenderSettings")
            if test_data.dim() != 5 or test_data.shape[1] != 1:
                raise ValueError("adversarial_test: with render=, test_data must be volumes [B, 1, D, H, W]")
            test_data = test_data.detach().float().contiguous()
            shown = lambda v: render_volumes(v[:, 0], render)[:, None]          # noqa: E731
            hw = tuple(test_data.shape[-2:])
            if elevation is not None:
                from ..physics.render import render_camera
                az = 0.0 if azimuth is None else azimuth
                shown = lambda v: render_camera(v[:, 0], az, elevation, render, differentiable=True).reshape(-1, 1, *hw)      # noqa: E731
            elif azimuth is not None:
                from ..physics.render import render_orbit
                shown = lambda v: render_orbit(v[:, 0], azimuth, render, differentiable=True).reshape(-1, 1, *hw)      # noqa: E731
            if evolve is not None:
                view = shown
                shown = lambda v: view(evolve(v))                               # noqa: E731
            if target is None:
                with torch.no_grad():
                    target = shown(test_data)
        elif evolve is not None:
            shown = evolve
            if target is None:
                from ..physics.render import render_volumes
                with torch.no_grad():
                    target = render_volumes(evolve(test_data)[:, 0].contiguous())[:, None]
        elif target is None:
            target = test_data
            if test_data.dim() == 5:
                from ..physics.render import render_volumes
                if test_data.shape[1] != 1:
                    raise ValueError("adversarial_test: volumes must be [B, 1, D, H, W]")
                target = render_volumes(test_data[:, 0].detach().float().contiguous())[:, None]
        sized = {}                           # the comparison image at the reconstruction's size, made once

        def compare_image(like):
            if target.shape[-2:] == like.shape[-2:]:
                return target
            if "t" not in sized:
                sized["t"] = F.adaptive_avg_pool2d(target, like.shape[-2:])
            return sized["t"]
        delta = torch.zeros_like(test_data, requires_grad=True)
        params = [p for p in model.parameters() if p.requires_grad]
        warned = model.__dict__.get("_warned_grad")
        try:
            for p in params:                 # no weight-gradient work at all, and nothing accumulates in the parameters' .grad
                p.requires_grad_(False)
            with warnings.catch_warnings():
                # the differentiable eval route is what this attack needs: SmokePhysNet's one-time hint about it does not apply here
                warnings.filterwarnings("ignore", message="SmokePhysNet: eval forward with autograd")
                for _ in range(num_steps):
                    with torch.enable_grad():
                        output = model(shown(torch.clamp(test_data + delta, 0, 1)))
                        loss = -F.mse_loss(output['reconstructed'], compare_image(output['reconstructed']))      # maximise the reconstruction error
                        (grad,) = torch.autograd.grad(loss, delta)
                    with torch.no_grad():
                        delta += epsilon / num_steps * torch.sign(grad)
                        delta.clamp_(-epsilon, epsilon)
        finally:
            for p in params:
                p.requires_grad_(True)
            if warned is None:
                model.__dict__.pop("_warned_grad", None)        # a later, unintended autograd forward still gets its hint
        if simulate is not None and not bool(torch.isfinite(delta).all()):
            raise RuntimeError("adversarial_test(simulate=): the perturbation is not finite.  The stepper's gradient on route='hip' holds "
                               "while every back-trace moves less than one cell (|dt * velocity| < 1); a grid past that one-cell limit "
                               "gets NaN gradients.  Use a smaller dt or FluidRollout(route='torch') / FluidRollout3D(route='torch').")
        with torch.no_grad():
            baseline = model(shown(test_data))
            adversarial_output = model(shown(torch.clamp(test_data + delta, 0, 1)))
            feature_stability = F.cosine_similarity(baseline['latent_features'], adversarial_output['latent_features'],
                                                    dim=1).mean().item()
        return {'adversarial_feature_stability': feature_stability,
                'adversarial_perturbation_norm': torch.norm(delta.detach()).item()}

    def physics_perturbation_test(self, model: nn.Module, simulator, num_tests: int = 50, *, batch_size: int = 64) -> Dict:
        """{'physics_prediction_stability', 'num_tests'} (perturbation_tests.py:100-146): 1 / (1 + mean over scenarios of the
        unbiased variance over 20 frames of physics_features, averaged over the 3 outputs).  `simulator` is an un-batched
        SmokeSimulator; its grid size, dt, viscosity and Jacobi sweeps define the scenarios."""
        if simulator.batch_size is not None:
            raise ValueError("physics_perturbation_test: pass an un-batched SmokeSimulator (batch_size=None); "
                             "the scenarios are batched internally")
        if num_tests < 1:
            raise ValueError(f"physics_perturbation_test: num_tests must be >= 1, got {num_tests}")
        ns = simulator.ns_solver
        scenarios = draw_scenarios(num_tests, ns.h, ns.w)
        _, features = self.perturbation_rollout(model, simulator, scenarios, batch_size=batch_size)
        variances = features.var(dim=1).mean(dim=1).tolist()         # per scenario: torch.var over the 20 frames, mean of 3
        return {'physics_prediction_stability': 1.0 / (1.0 + np.mean(variances)), 'num_tests': num_tests}

    def perturbation_rollout(self, model: nn.Module, simulator, scenarios, *, batch_size: int = 64):
        """The simulation and model half of physics_perturbation_test for given scenarios (lists of (x, y, intensity), as
        draw_scenarios returns): returns frames [num_tests, 20, H, W] (the fractal-perturbed densities simulate_step would emit)
        and physics_features [num_tests, 20, 3].  Leaves `simulator` as the reference's loop would: u, v, p, density equal
        to the last scenario's final state, history extended by the frames in scenario order (trimmed to max_history)."""
        if simulator.batch_size is not None:
            raise ValueError("perturbation_rollout: pass an un-batched SmokeSimulator (batch_size=None)")
        model.eval()
        ns = simulator.ns_solver
        T, steps = len(scenarios), 20
        sim = SmokeSimulator(ns.grid_size, dt=ns.dt, viscosity=ns.viscosity, device=ns.device, batch_size=T,
                             jacobi_iters=ns.jacobi_iters)
        for g, sources in enumerate(scenarios):
            for x, y, intensity in sources:                          # one source at a time, in draw order, as the reference adds them
                sim.add_incense_source([(x, y)], [intensity], grid=g)
        frames = sim.simulate_sequence(steps, add_fractal=True)      # [T, 20, H, W]
        H, W = frames.shape[2:]
        features = _chunked_forward(model, frames.view(T * steps, 1, H, W), batch_size, ('physics_features',))['physics_features']
        # the caller's simulator: the state and history the serial loop would have left
        last = sim.ns_solver
        ns.u, ns.v, ns.p, ns.density = last.u[-1], last.v[-1], last.p[-1], last.density[-1]
        ns.boundary.zero_()                                          # (setup_grid's other effect)
        keep = min(simulator.max_history, T * steps)
        simulator.history.extend(f.clone() for f in frames.view(T * steps, H, W)[T * steps - keep:])
        del simulator.history[:max(0, len(simulator.history) - simulator.max_history)]
        ns.check()
        sim.ns_solver.close()
        return frames, features.view(T, steps, -1)
