"""The yardstick of the patch-correlation tests: the homography / patch-correlation part of the reference's photometric branch
(scripts/main.py:783-851) restated in float64 from its description -- patch grid, per-view homography, the align-corners map followed by
grid_sample's align_corners=False, gray AFTER sampling, torch.cov, sqrt(var var + 1e-12), torch.topk, torch.nanmean -- with torch's own
operators.  The branch is inline in main.py and cannot be imported; nothing of it is copied or executed.  `dtype` lets the same code run in
float32: the distance between the two runs is the yardstick's own sensitivity to rounding.

Also here: the seeded scenes of the tests, the tie gap of a ray's selection and the share of samples next to a pixel border.
No test in this file."""
import math

import torch
import torch.nn.functional as F

from vsrd_amd.synthetic import kitti_intrinsics

GRAY_WEIGHTS = (0.2989, 0.587, 0.114)


def patch_grid(patch_size, dtype=torch.float64, device=None):
    """[ph,pw,2] offsets (dx, dy): arange(size) - size // 2 per axis, meshgrid(indexing="xy"), x the fast index."""
    axes = [torch.arange(size, dtype=dtype, device=device) - size // 2 for size in patch_size]
    return torch.stack(torch.meshgrid(*axes, indexing="xy"), dim=-1)


def homographies(K, E, target, positions, normals):
    """[V,R,3,3]: K_s (R_s R_t^T - R_s (R_s^T t_s - R_t^T t_t) n^T / -(n^T p)) K_t^-1 for every view s, the target included."""
    Kt, Rt, tt = K[target], E[target, :3, :3], E[target, :3, 3:]
    nT, p = normals.unsqueeze(-2), positions.unsqueeze(-1)                       # [R,1,3], [R,3,1]
    out = []
    for Ks, Es in zip(K, E):
        Rs, ts = Es[:3, :3], Es[:3, 3:]
        out.append(Ks @ (Rs @ Rt.T - Rs @ (Rs.T @ ts - Rt.T @ tt) @ nT / -(nT @ p)) @ torch.linalg.inv(Kt))
    return torch.stack(out, dim=0)


def source_coordinates(K, E, target, pixels, positions, normals, patch_size):
    """[V,R,P,2]: the patch pixels of every ray in every view, s = h_xy / (h_z + 1e-6), in the views' pixel units."""
    grid = patch_grid(patch_size, positions.dtype, positions.device)
    q = pixels.to(positions.dtype).unsqueeze(-2).unsqueeze(-3) + grid            # [R,ph,pw,2]
    q = F.pad(q, (0, 1), mode="constant", value=1.0).flatten(1, 2)               # [R,P,3]
    h = torch.einsum("vrmn,rpn->vrpm", homographies(K, E, target, positions, normals), q)
    return h[..., :-1] / (h[..., -1:] + 1e-6)


def sample_pixel_coordinates(coordinates, height, width):
    """What grid_sample makes of the reference's normalised grid: s W / (W - 1) - 0.5 (and y)."""
    size = torch.tensor([width, height], dtype=coordinates.dtype, device=coordinates.device)
    return coordinates * size / (size - 1) - 0.5


def sample_patches(images, coordinates, gray_first=False):
    """images [V,3,H,W], coordinates [V,R,P,2] -> gray patches [V,R,P]: linear_map [0, size-1] -> [-1, 1], grid_sample(bilinear, zeros,
    align_corners=False), then 0.2989 r + 0.587 g + 0.114 b.  `gray_first`: the same with the gray map before the interpolation."""
    H, W = images.shape[-2:]
    upper = torch.tensor([W - 1, H - 1], dtype=coordinates.dtype, device=coordinates.device)
    grid = -1.0 + 2.0 * (coordinates - 0.0) / (upper - 0.0)
    weights = torch.tensor(GRAY_WEIGHTS, dtype=images.dtype, device=images.device).view(1, 3, 1, 1)
    if gray_first:
        return F.grid_sample((images * weights).sum(dim=1, keepdim=True), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
    sampled = F.grid_sample(images, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return (sampled * weights).sum(dim=1)


def corrcoef(inputs, epsilon=1e-12):
    covariances = torch.cov(inputs)
    variances = torch.diag(covariances)
    return covariances / torch.sqrt(variances.unsqueeze(-1) * variances.unsqueeze(0) + epsilon)


def correlate(patches, converged, top_k=4, record=True):
    """Steps 5-6 on patches [V,R,P]: -> (loss, coefficients [R,V,V], indices [R,V,k] of the selection).  Rows of unconverged rays are
    zero / -1 (`record` False: neither is filled in).  No converged ray: loss 0 (the reference adds no term; the device op's stated
    deviation)."""
    V, R, _ = patches.shape
    coefficients = torch.zeros(R, V, V, dtype=patches.dtype)
    indices = torch.full((R, V, top_k), -1, dtype=torch.int64)
    chosen = []
    for ray in torch.nonzero(converged.reshape(-1)).flatten().tolist():
        matrix = corrcoef(patches[:, ray])
        top = torch.topk(matrix, k=top_k, dim=-1)
        if record:
            coefficients[ray], indices[ray] = matrix.detach(), top.indices
        chosen.append(top.values)
    if not chosen:
        return patches.sum() * 0.0, coefficients, indices
    return (1.0 - torch.nanmean(torch.cat(chosen, dim=0))) / 2.0, coefficients, indices


def reference(images, K, E, pixels, positions, normals, converged, patch_size=(11, 11), top_k=4, target=0, dtype=torch.float64, record=True):
    """Steps 1-6, on the device of its inputs.  pixels [R,2] integer (x, y).  -> dict(loss, patches [V,R,P], coefficients, indices, coordinates [V,R,P,2] in pixels of
    the SAMPLED image, i.e. after the W / (W - 1) - 0.5 map)."""
    images, K, E = images.to(dtype), K.to(dtype), E.to(dtype)
    positions, normals = positions.to(dtype), normals.to(dtype)
    coordinates = source_coordinates(K, E, target, pixels, positions, normals, patch_size)
    patches = sample_patches(images, coordinates)
    loss, coefficients, indices = correlate(patches, converged.reshape(-1), top_k, record)
    H, W = images.shape[-2:]
    return dict(loss=loss, patches=patches, coefficients=coefficients, indices=indices, coordinates=sample_pixel_coordinates(coordinates.detach(), H, W))


def reference_gradients(images, K, E, pixels, positions, normals, converged, patch_size=(11, 11), top_k=4, target=0, dtype=torch.float64):
    """float64 (or `dtype`) autograd of the loss: -> (loss, d loss / d positions, d loss / d normals)."""
    p, n = positions.to(dtype).clone().requires_grad_(True), normals.to(dtype).clone().requires_grad_(True)
    loss = reference(images, K, E, pixels, p, n, converged, patch_size, top_k, target, dtype)["loss"]
    gp, gn = torch.autograd.grad(loss, [p, n], allow_unused=True)
    zero = torch.zeros_like(p)
    return loss.detach(), zero if gp is None else gp, zero if gn is None else gn


def tie_gaps(coefficients, top_k):
    """[R]: per ray the smallest difference between the k-th and (k+1)-th largest coefficient over its rows (NaN ranks first; k == V: inf)."""
    R, V, _ = coefficients.shape
    if top_k >= V:
        return torch.full((R,), float("inf"), dtype=torch.float64)
    ranked = torch.nan_to_num(coefficients.double(), nan=1e30).sort(dim=-1, descending=True).values
    return (ranked[..., top_k - 1] - ranked[..., top_k]).min(dim=-1).values


def row_tie_gaps(coefficients, top_k):
    """[R,V]: the same per row."""
    R, V, _ = coefficients.shape
    if top_k >= V:
        return torch.full((R, V), float("inf"), dtype=torch.float64)
    ranked = torch.nan_to_num(coefficients.double(), nan=1e30).sort(dim=-1, descending=True).values
    return ranked[..., top_k - 1] - ranked[..., top_k]


def border_share(coordinates):
    """The share of samples within 1e-3 px of a pixel border (where the bilinear interpolant's slope jumps)."""
    finite = torch.nan_to_num(coordinates.double(), nan=0.5, posinf=0.5, neginf=0.5)
    near = (finite - finite.round()).abs() < 1e-3
    return near.any(dim=-1).double().mean().item()


def taps_outside(coordinates, height, width):
    """[R] bool: some sample of the ray, in some view, has one of its four taps outside the image (or is not finite)."""
    x, y = coordinates[..., 0], coordinates[..., 1]
    inside = (x >= 0) & (x <= width - 1) & (y >= 0) & (y <= height - 1)
    return (~inside).any(dim=-1).any(dim=0)


def selection_mask(indices, V):
    """indices [R,V,k] -> int64 [R,V]: bit j of entry (r, i) set when j is among row i's selection (the device's `selected`)."""
    bits = torch.zeros(indices.shape[:2], dtype=torch.int64)
    for slot in range(indices.shape[-1]):
        column = indices[..., slot]
        bits |= torch.where(column >= 0, torch.ones_like(column) << column.clamp_min(0), torch.zeros_like(column))
    return bits


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def cameras(V, height, width, baseline=5.0):
    """KITTI-360 intrinsics scaled to the image; target (view 0) extrinsics the identity; the sources alternate before and behind it along z,
    evenly spaced over `baseline` metres in all, with the synthetic trajectory's yaw of 0.5 degrees per metre."""
    K = kitti_intrinsics(height, width).expand(V, 3, 3).contiguous()
    E = torch.eye(4).repeat(V, 1, 1)
    half = max((V - 1 + 1) // 2, 1)
    offsets = [0.0] + [sign * i * (baseline / 2.0) / half for i in range(1, half + 1) for sign in (1.0, -1.0)]
    for v, k in enumerate(offsets[:V]):
        yaw = math.radians(0.5 * k)
        E[v, :3, :3] = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
        E[v, 2, 3] = k
    return K, E


def noise_images(generator, V, height, width):
    return torch.rand(V, 3, height, width, generator=generator)


def smooth_images(generator, V, height, width):
    """A sum of six sinusoids of period >= 24 px per view and channel, scaled into [0,1]."""
    y, x = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
    images = torch.zeros(V, 3, height, width)
    for _ in range(6):
        period = torch.empty(V, 3, 1, 1).uniform_(24.0, 64.0, generator=generator)
        angle = torch.empty(V, 3, 1, 1).uniform_(0.0, 2.0 * math.pi, generator=generator)
        phase = torch.empty(V, 3, 1, 1).uniform_(0.0, 2.0 * math.pi, generator=generator)
        images += torch.sin(2.0 * math.pi * (x * torch.cos(angle) + y * torch.sin(angle)) / period + phase)
    return (images / 12.0 + 0.5).clamp(0.0, 1.0)


def draw_rays(generator, R, K, height, width, patch_size=(11, 11)):
    """Pixels whose patch, magnified 1.5 times about the principal point (the nearest source at the nearest depth magnifies by 1.45), stays
    inside the image; positions 8-28 m along the pixel's ray; normals facing the camera with noise."""
    def axis(centre, size, half):
        lo, hi = math.ceil(centre - (centre - 1.0) / 1.5 + half), math.floor(centre + (size - 2.0 - centre) / 1.5 - half)
        lo = min(max(lo, 0), size - 1)
        return torch.randint(lo, max(hi, lo) + 1, (R,), generator=generator)
    x = axis(K[0, 0, 2].item(), width, (patch_size[0] + 1) // 2)
    y = axis(K[0, 1, 2].item(), height, (patch_size[1] + 1) // 2)
    pixels = torch.stack([x, y], dim=-1)
    depth = torch.empty(R, 1).uniform_(8.0, 28.0, generator=generator)
    rays = (torch.linalg.inv(K[0].double()) @ F.pad(pixels.double(), (0, 1), value=1.0).T).T.float()
    positions = rays * depth
    normals = F.normalize(-F.normalize(positions, dim=-1) + 0.3 * torch.randn(R, 3, generator=generator), dim=-1)
    return pixels, positions, normals


def scene(seed, V, R, height, width, smooth=False, baseline=5.0, patch_size=(11, 11)):
    """-> dict(images [V,3,H,W], K, E, pixels [R,2] int64, positions, normals [R,3] float32, converged [R] bool all True)."""
    generator = torch.Generator().manual_seed(seed)
    K, E = cameras(V, height, width, baseline)
    images = (smooth_images if smooth else noise_images)(generator, V, height, width)
    pixels, positions, normals = draw_rays(generator, R, K, height, width, patch_size)
    return dict(images=images, K=K, E=E, pixels=pixels, positions=positions, normals=normals, converged=torch.ones(R, dtype=torch.bool), generator=generator)


def redraw_rays(s, patch_size, top_k, min_gap=1e-4, rounds=8):
    """Gradient scenes: re-draw (on the CPU, before anything runs) the rays whose tie gap is below `min_gap` or whose patches have a tap
    outside the image -- zero patches tie at exactly 0 and their gradient is scaled by 1 / sqrt(1e-12).  -> the share of rays re-drawn
    (a ray re-drawn twice counts once); rays still bad after `rounds` stay counted and the caller's cap catches them."""
    H, W = s["images"].shape[-2:]
    R = s["pixels"].shape[0]
    redrawn = torch.zeros(R, dtype=torch.bool)
    for _ in range(rounds):
        out = reference(s["images"], s["K"], s["E"], s["pixels"], s["positions"], s["normals"], s["converged"], patch_size, top_k)
        bad = (tie_gaps(out["coefficients"], top_k) < min_gap) | taps_outside(out["coordinates"], H, W)
        if not bool(bad.any()):
            break
        redrawn |= bad
        pixels, positions, normals = draw_rays(s["generator"], R, s["K"], H, W, patch_size)
        s["pixels"] = torch.where(bad[:, None], pixels, s["pixels"])
        s["positions"] = torch.where(bad[:, None], positions, s["positions"])
        s["normals"] = torch.where(bad[:, None], normals, s["normals"])
    return redrawn.double().mean().item()
