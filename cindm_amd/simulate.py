"""Re-simulation of sampled n-body designs on the device, and the metrics the reference's 1-D script derives from it.

``simulation`` stands where the reference calls ``utils.simulation`` (utils.py:1071-1125) and keeps its signature, so
``eval_simu(..., simulation=cindm_amd.simulation)`` works as written.  One launch of ``nbody_simulate_kernel``
(csrc/nbody.h, C entry ``cindm_nbody_simulate``) advances the whole batch; DESIGN 4.10b states the rule.

What it is: the continuous-time dynamics of the scene ``add_body`` / ``add_walls`` build (utils.py:1009-1033) -- equal, frictionless,
perfectly elastic discs in a box, no gravity, no damping -- with every wall and pair contact found in closed form and resolved at
its own time, in float64.  What it is NOT: an emulation of Chipmunk's step, which pymunk runs for the reference.  Chipmunk detects
contacts once per 1/60 s and corrects penetration over several steps, so its trajectories differ from these by about one step's
travel (``|v| * dt``, about 2 px at the data generator's speeds) per contact.  That difference has not been measured (pymunk is not
available where this was written), and no equality with the paper's numbers is claimed: a user who has pymunk passes the reference's
simulator to ``eval_simu`` / ``design_report`` and compares.

``design_report`` does what inference/inverse_design_diffusion_1d.py:316-340 does after sampling."""
import ctypes as C
import math

import torch

from . import _ffi
from .data_utils import eval_simu

MAX_BODIES = 8
MAX_STEPS = 65535
MAX_BATCH = 1 << 22
MAX_EVENTS = 4096


def simulation(features, n_steps, filename=None, width=200, height=200, radius=20, mass=1, *, wall_radius=1.0, dt=1 / 60,
               max_events_per_frame=64, return_status=False):
    """``features`` [B, n_bodies, 4] = (x, y, vx, vy) in simulator units -> float64 [B, n_steps, n_bodies, 4] on the device; frame i is
    the state at time ``i * dt``, frame 0 the input (the reference's ``run_simulation`` records before it steps, utils.py:1052-1060).

    ``features``: any floating dtype, converted exactly to float64; any strides; a CPU tensor is moved to the current ROCm device.
    ``n_bodies`` <= 8.  ``mass`` must be a positive scalar and is otherwise unused: equal masses cancel.  ``filename`` must be None
    (nothing is rendered).  ``wall_radius`` is the half-thickness of the reference's wall segments (1), ``max_events_per_frame`` the
    bound on contacts resolved inside one frame (the rest of such a frame is ballistic).
    ``return_status=True`` also returns ``(status, events)``, int32 [B] on the device: status bit 1 = the input starts with an overlap or
    a centre outside the box, 2 = the event cap was reached in some frame, 4 = coincident centres at a pair contact (skipped), 8 = a
    non-finite input (that design's rows are NaN); events = contacts resolved.

    Continuous-time dynamics, not Chipmunk's discretisation: see the module docstring.  Argument errors are ValueError /
    NotImplementedError before any device work; without a ROCm device the call raises CindmError (there is no CPU execution path).
    The launch is asynchronous on the current stream of the features' device."""
    if filename is not None:
        raise NotImplementedError("simulation: filename= asks for the reference's rendering and .npy dump; nothing is rendered here "
                                  "(pass filename=None and save the returned tensor)")
    features = torch.as_tensor(features)
    if features.dim() != 3 or features.shape[2] != 4:
        raise ValueError(f"simulation: features must be [batch, n_bodies, 4] = (x, y, vx, vy), got {tuple(features.shape)}")
    if not features.is_floating_point():
        raise ValueError(f"simulation: features must be a floating-point tensor, got {features.dtype}")
    B, nb = int(features.shape[0]), int(features.shape[1])
    if not 1 <= nb <= MAX_BODIES:
        raise ValueError(f"simulation: n_bodies must be in 1 .. {MAX_BODIES}, got {nb}")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"simulation: batch must be in 1 .. 2^22, got {B}")
    if isinstance(n_steps, bool) or int(n_steps) != n_steps or not 1 <= int(n_steps) <= MAX_STEPS:
        raise ValueError(f"simulation: n_steps must be an integer in 1 .. {MAX_STEPS}, got {n_steps!r}")
    n_steps = int(n_steps)
    try:
        width, height, radius, wall_radius, dt, mass = (float(v) for v in (width, height, radius, wall_radius, dt, mass))
    except (TypeError, ValueError) as e:
        raise ValueError(f"simulation: width, height, radius, mass, wall_radius and dt must be scalars ({e})") from e
    if not (mass > 0 and math.isfinite(mass)):
        raise ValueError(f"simulation: mass must be a positive scalar (equal masses cancel), got {mass}")
    if not (radius > 0 and wall_radius >= 0 and math.isfinite(radius) and math.isfinite(wall_radius)):
        raise ValueError(f"simulation: radius must be positive and wall_radius non-negative, got {radius}, {wall_radius}")
    lo = radius + wall_radius
    if not (math.isfinite(width) and math.isfinite(height) and width - radius - wall_radius > lo and height - radius - wall_radius > lo):
        raise ValueError(f"simulation: a {width} x {height} box leaves no room for a centre of a disc of radius {radius} "
                         f"(walls of half-thickness {wall_radius})")
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError(f"simulation: dt must be positive and finite, got {dt}")
    if isinstance(max_events_per_frame, bool) or int(max_events_per_frame) != max_events_per_frame or \
            not 1 <= int(max_events_per_frame) <= MAX_EVENTS:
        raise ValueError(f"simulation: max_events_per_frame must be an integer in 1 .. {MAX_EVENTS}, got {max_events_per_frame!r}")
    if not features.is_cuda:
        if not torch.cuda.is_available():
            raise _ffi.CindmError("simulation needs a ROCm device; there is no CPU execution path")
        features = features.to(torch.device("cuda", torch.cuda.current_device()))
    device = features.device
    with torch.cuda.device(device):
        f64 = features.to(torch.float64).contiguous()          # on the current stream: ordered after the producer of features
        out = torch.empty((B, n_steps, nb, 4), dtype=torch.float64, device=device)
        status = torch.empty((B,), dtype=torch.int32, device=device)
        events = torch.empty((B,), dtype=torch.int32, device=device)
        desc = _ffi.NBodyDesc(width, height, radius, wall_radius, dt, int(max_events_per_frame))
        _ffi.check(_ffi.lib().cindm_nbody_simulate(C.byref(desc), _ffi.ptr(f64), B, nb, n_steps, _ffi.ptr(out), _ffi.ptr(status),
                                                   _ffi.ptr(events), _ffi.current_stream(device)))
    return (out, (status, events)) if return_status else out


_device_simulation = simulation


def design_report(pred, eval_fn, n_bodies, start_eval_t, output_steps, *, eval_fn_std=None, time_interval=4, simulation=simulation):
    """What the reference's script computes from a sampled batch (inference/inverse_design_diffusion_1d.py:316-340): re-simulate every
    design from frame ``start_eval_t`` of ``pred`` for ``output_steps - 1`` model steps, score the re-simulation, and measure how far
    the sampled trajectory is from it.

    ``pred`` [batch, start_eval_t + output_steps, n_bodies * 4] in diffusion units (what ``sample`` returns).  Returns a dict:
    ``pred_simu`` [batch, output_steps - 1, n_bodies * 4], ``design_obj_simu`` = eval_fn(pred_simu), ``design_obj_simu_CI`` =
    eval_fn_std(pred_simu) * 1.96 / sqrt(batch) when ``eval_fn_std`` is given, ``RMSE`` / ``RMSE_CI`` (per-design root mean square of
    [pred[:, :start_eval_t + 1], pred_simu] - pred: mean, and std * 1.96 / sqrt(batch)), ``MAE`` / ``MAE_CI`` likewise on absolute
    differences (0-dim tensors on pred's device, float64 when the simulator returns float64), and ``n_flagged``: the count of designs
    with a non-zero simulator status -- an int with ``cindm_amd.simulation``, None with any other ``simulation=`` callable (which
    reports none).  Everything goes through ``eval_simu``; with the default simulator nothing leaves the device but ``n_flagged``.
    The default simulator is not Chipmunk (module docstring): these are not the paper's numbers."""
    if pred.dim() != 3 or pred.shape[2] != 4 * n_bodies:
        raise ValueError(f"design_report: pred must be [batch, steps, {4 * n_bodies}], got {tuple(pred.shape)}")
    if start_eval_t < 0 or output_steps < 2 or pred.shape[1] != start_eval_t + output_steps:
        raise ValueError(f"design_report: pred has {pred.shape[1]} steps, start_eval_t + output_steps = {start_eval_t + output_steps} "
                         "(output_steps >= 2, start_eval_t >= 0)")
    batch = pred.shape[0]
    flagged = []
    own = simulation is _device_simulation

    def simulate(features, n_steps):
        if not own:
            return simulation(features=features, n_steps=n_steps)
        out, (status, _) = simulation(features=features, n_steps=n_steps, return_status=True)
        flagged.append(status)
        return out

    pred_simu, design_obj_simu = eval_simu(pred[:, start_eval_t:start_eval_t + 1], eval_fn, n_bodies, output_steps - 1, time_interval,
                                           simulation=simulate)
    rep = {"pred_simu": pred_simu, "design_obj_simu": design_obj_simu}
    if eval_fn_std is not None:
        rep["design_obj_simu_CI"] = eval_fn_std(pred_simu) * 1.96 / math.sqrt(batch)
    diff = torch.cat([pred[:, :start_eval_t + 1].to(pred_simu.dtype), pred_simu], 1) - pred
    rms = diff.square().mean((1, 2)).sqrt()
    mae = diff.abs().mean((1, 2))
    rep["RMSE"] = rms.mean()
    rep["RMSE_CI"] = rms.std() * 1.96 / math.sqrt(batch)
    rep["MAE"] = diff.abs().mean()
    rep["MAE_CI"] = mae.std() * 1.96 / math.sqrt(batch)
    rep["n_flagged"] = int((flagged[0] != 0).sum()) if own else None
    return rep
