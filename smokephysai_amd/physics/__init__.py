from .navier_stokes import NavierStokesSimulator
from .navier_stokes3d import NavierStokesSimulator3D
from .smoke_simulator import SmokeSimulator
from .smoke_simulator3d import SmokeSimulator3D
from .fractal_generator import FractalGenerator
from .render import (RenderSettings, camera_backward_supported, camera_backward_workspace, camera_samples, camera_supported, camera_workspace, orbit_backward_workspace, orbit_samples, orbit_supported,
                     orbit_workspace,
                     render_backward_workspace, render_camera, render_orbit, render_supported, render_volumes, render_workspace)
from .fluid_grad import Branches, FluidRollout, advect_rule, buoy_diffuse_rule, fluid_rollout, fluid_step, fluid_step_rule, project_rule
from .fluid_grad3d import (FluidRollout3D, advect3d_rule, buoy_diffuse3d_rule, fluid_rollout3d, fluid_step3d, fluid_step3d_rule,
                           project3d_rule)
from .fluid_tangent import (FlowChaos, LyapunovResult, flow_chaos, fluid_step_jvp, fluid_step_jvp_rule, fluid_tangent_rollout,
                            kaplan_yorke_dimension, ks_entropy, lyapunov_exponents)
from .fluid_tangent3d import flow_chaos3d, fluid_step3d_jvp, fluid_step3d_jvp_rule, fluid_tangent_rollout3d, lyapunov_exponents3d
from .flow_map import FtleResult, flow_ftle, flow_ftle_rule, flow_map_step, flow_map_step_rule, ftle_field, ftle_rule
from .flow_map3d import flow_ftle3d, flow_ftle3d_rule, flow_map_step3d, flow_map_step3d_rule, ftle3d_rule, ftle_field3d

__all__ = ["flow_ftle3d", "flow_ftle3d_rule", "flow_map_step3d", "flow_map_step3d_rule", "ftle3d_rule", "ftle_field3d",
           "FtleResult", "flow_ftle", "flow_ftle_rule", "flow_map_step", "flow_map_step_rule", "ftle_field", "ftle_rule", "FlowChaos", "flow_chaos", "flow_chaos3d", "kaplan_yorke_dimension", "ks_entropy", "fluid_step3d_jvp", "fluid_step3d_jvp_rule", "fluid_tangent_rollout3d", "lyapunov_exponents3d", "LyapunovResult", "fluid_step_jvp", "fluid_step_jvp_rule", "fluid_tangent_rollout", "lyapunov_exponents", "Branches", "FluidRollout", "FluidRollout3D", "advect3d_rule", "buoy_diffuse3d_rule", "fluid_rollout3d", "fluid_step3d",
           "fluid_step3d_rule", "project3d_rule", "advect_rule", "buoy_diffuse_rule", "fluid_rollout", "fluid_step", "fluid_step_rule", "project_rule", "NavierStokesSimulator", "NavierStokesSimulator3D", "SmokeSimulator", "SmokeSimulator3D", "FractalGenerator", "RenderSettings",
           "camera_backward_supported", "camera_backward_workspace", "camera_samples", "camera_supported", "camera_workspace", "orbit_backward_workspace", "orbit_samples", "orbit_supported",
           "orbit_workspace",
           "render_backward_workspace", "render_camera", "render_orbit", "render_supported", "render_volumes", "render_workspace"]
