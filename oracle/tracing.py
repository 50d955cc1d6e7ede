"""Oracle: sphere tracing (TEST INFRASTRUCTURE).

Restates ``vsrd/rendering/renderers.py:10-18`` (entry point of a ray into the origin-centred bounding sphere) and
``renderers.py:32-57`` (the march) for a field given as a callable ``positions [R,3] -> distances [R]``.

The reference keeps three tensors per ray -- position, foreground, converged -- and in every iteration
  1. evaluates the field at every position,
  2. moves the rays that are foreground and were NOT converged by the previous iteration,
  3. clears the foreground flag of every ray that is now on or beyond the sphere (sticky),
  4. OVERWRITES converged with ``|distance of step 1| < criteria`` -- a ray converged by iteration k stays put in k + 1 and is then judged
     by the distance at the point it was moved to in k; a ray that stepped past a rim may un-converge and walk on,
  5. leaves the loop when every ray of the batch is non-foreground or converged (``early_exit``).
Step 5 makes a ray's result depend on the other rays of the call; without it (``early_exit=False``) the march is a function of the ray alone,
which is the contract of ``vsrd_sphere_trace``.  The two agree because the stationary state is a fixed point: a ray that did not move
in an iteration and may not move in the next sees the same distance again, for ever -- which is also why that form may stop evaluating
once EVERY ray is stationary (the same batch at the same points gives the same bits).

``stop_at_first_convergence`` is the rule the kernels had before: a ray is frozen, flag included, the first time it is non-foreground
or converged after an iteration.  It is kept so that fixtures can show that they tell the two apart.
"""
from typing import NamedTuple

import torch

BORDERLINE = 1.0e-4    # relative band around a threshold inside which float32 and float64 may decide differently


class TraceOutput(NamedTuple):
    positions: torch.Tensor        # [R,3]
    converged: torch.Tensor        # [R] bool   the reference's convergence_masks
    foreground: torch.Tensor       # [R] bool   the foreground flags after the last iteration
    criteria_gap: torch.Tensor     # [R]        min over the evaluations of | |sdf| - criteria |      (inf: never evaluated)
    radius_gap: torch.Tensor       # [R]        min over the moves of | |p| - radius | while foreground (inf: no sphere)
    live_iterations: torch.Tensor  # [R] int64  iterations until the ray is stationary (what a per-ray march evaluates)
    iterations: int                #            iterations the batch ran


def sphere_entry(origins, directions, bounding_radius):
    """renderers.py:10-18 -> (distance to the entry point [R], hit [R])."""
    a = (directions * directions).sum(-1)
    b = (directions * origins).sum(-1)
    c = (origins * origins).sum(-1) - bounding_radius ** 2.0
    discriminant = b ** 2.0 - a * c
    return (-b - torch.sqrt(discriminant)) / a, discriminant >= 0.0


def trace(field_distance, origins, directions, num_iterations, criteria, foreground=None, bounding_radius=None, initialise=True,
          early_exit=True, stop_at_first_convergence=False):
    """origins [R,3] or [3], directions [R,3] (any length), foreground [R] bool or None (= finite origins); works in the dtype of
    ``directions``.  ``bounding_radius`` None or 0: no sphere."""
    dtype = directions.dtype
    positions = origins.to(dtype).expand_as(directions).clone()
    R = positions.shape[0]
    foreground = torch.isfinite(positions).all(-1) if foreground is None else foreground.reshape(R).bool().clone()
    if bounding_radius and initialise:
        distance, hit = sphere_entry(positions, directions, bounding_radius)
        positions = torch.where(hit[:, None], positions + directions * distance[:, None], positions)
        foreground = foreground & hit
    converged = torch.zeros(R, dtype=torch.bool)
    frozen = torch.zeros(R, dtype=torch.bool)              # stop_at_first_convergence only
    stationary = torch.zeros(R, dtype=torch.bool)
    criteria_gap = torch.full((R,), float("inf"), dtype=dtype)
    radius_gap = torch.full((R,), float("inf"), dtype=dtype)
    live_iterations = torch.zeros(R, dtype=torch.int64)
    iterations = 0
    with torch.no_grad():
        for _ in range(num_iterations):
            if not early_exit and not stop_at_first_convergence and bool(stationary.all()):
                break                                       # every ray is at its fixed point: the remaining iterations change nothing
            sdf = field_distance(positions).reshape(R)
            iterations += 1
            live_iterations += (~stationary).long()
            move = foreground & ~converged & ~frozen
            positions = torch.where(move[:, None], positions + directions * sdf[:, None], positions)
            if bounding_radius:
                norm = torch.linalg.norm(positions, dim=-1)
                radius_gap = torch.where(foreground & ~frozen, torch.minimum(radius_gap, (norm - bounding_radius).abs()), radius_gap)
                foreground = torch.where(frozen, foreground, foreground & (norm < bounding_radius))
            criteria_gap = torch.where(frozen, criteria_gap, torch.minimum(criteria_gap, (sdf.abs() - criteria).abs()))
            converged = torch.where(frozen, converged, sdf.abs() < criteria)
            stationary = stationary | (~move & ~(foreground & ~converged))
            if stop_at_first_convergence:
                frozen = frozen | ~foreground | converged
            if early_exit and bool((~foreground | converged).all()):
                break
    return TraceOutput(positions, converged, foreground, criteria_gap, radius_gap, live_iterations, iterations)


def borderline(out, criteria, bounding_radius=None, band=BORDERLINE):
    """Rays with a decision anywhere along their path inside the relative band of its threshold."""
    near = out.criteria_gap <= band * criteria
    if bounding_radius:
        near = near | (out.radius_gap <= band * bounding_radius)
    return near
