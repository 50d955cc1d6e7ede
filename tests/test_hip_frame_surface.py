"""vsrd_frame_surface (csrc/frame_surface.h) on the GPU, link by link against the composition of what the project already pins --
vsrd_sphere_trace, vsrd_field_eval, rendering.shadow_rendering and rendering.phong_shading -- on what the kernel itself exports; then
batches with headers, capture, refusals, and FrameOptimizer / FrameBatch.surface().

The scenes were chosen with the CPU oracle (oracle/tracing.py) so that in every case at least a quarter of the pixels converge, at least a
quarter do not, at least one run of 64 pixels is empty, and at least one converged pixel is shadowed and one lit; every case asserts those
conditions on the composition it is checked against."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from frame_rows import RowArena

pytestmark = pytest.mark.gpu

TRACE = (128, 0.01, 50.0)                 # iterations, convergence criterion, bounding radius
T = 0.3
CAMERA = (0.0, -3.0, 0.0)
LIGHT = (1.0, 0.8, 0.3)                   # the direction the light travels: from above and the left
SIZES = ((6, 76), (5, 20))                # a full run plus a 12-pixel tail, rows of 10 bytes; a row shorter than a run, rows of 3 bytes
ULP = 2.0 ** -23
SHADING = dict(shininess=8.0, background_color=(0.2, 0.4, 0.6), light_ambient=(0.9, 0.8, 0.7), light_diffuse=(1.0, 0.9, 0.8), light_specular=(0.7, 0.8, 0.9),
               material_ambient=(0.1, 0.2, 0.1), material_specular=(0.5, 0.4, 0.3), material_emission=(0.02, 0.01, 0.03))
# (N, H, W) -> horizontal and vertical pitch of the pixels' slopes and the slope of the image centre
VIEWS = {(3, 6, 76): (1 / 40, 0.16, 0.0, 0.42), (3, 5, 20): (1 / 10, 0.2, 0.0, 0.4), (1, 6, 76): (1 / 150, 0.09, -0.19, 0.38), (1, 5, 20): (1 / 40, 0.1, -0.19, 0.36),
         (4, 6, 76): (1 / 40, 0.16, 0.0, 0.42), (2, 6, 76): (1 / 40, 0.16, 0.0, 0.42)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def scene(N):
    """A slab seen from above with two boxes (and a third, small one for N = 4) standing on it; N = 1: the first box alone, N = 2: slab and box.
    (The slab is 1.2 m thick: a residual field's surface lies some 0.27 m INSIDE its box, and a thinner slab would have none.)"""
    loc = torch.tensor([[0.0, 2.0, 10.0], [-1.6, 0.5, 8.5], [1.9, 0.7, 10.5], [0.2, 1.0, 7.0]])
    dim = torch.tensor([[5.0, 0.6, 5.0], [0.8, 0.9, 0.8], [0.6, 0.7, 1.0], [0.3, 0.4, 0.3]])
    yaw = torch.tensor([0.0, 0.5, -0.4, 0.9])
    keep = slice(1, 2) if N == 1 else slice(0, N)
    loc, dim, yaw = loc[keep], dim[keep], yaw[keep]
    rot = torch.stack([torch.stack([torch.cos(yaw), torch.zeros(N), torch.sin(yaw)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                       torch.stack([-torch.sin(yaw), torch.zeros(N), torch.cos(yaw)], -1)], -2)
    return loc, dim, rot


def instances_of(dev, N):
    from vsrd_amd import fields
    loc, dim, rot = scene(N)
    return fields.pack_instances(loc, rot, dim).to(dev)


def mlp_of(dev, N, seed=11):
    """Small random MLP weights, centred (rendering._centre_mlp_torch): the residual is close to sigmoid(-1) everywhere, the surface a rounded box."""
    from vsrd_amd.rendering import renderers
    from vsrd_amd import _lib
    g = torch.Generator().manual_seed(seed)
    return renderers._centre_mlp_torch(0.05 * torch.randn(N, _lib.MLP_WEIGHTS, generator=g)).contiguous().to(dev)


def rays(N, H, W):
    px, py, sx, sy = VIEWS[(N, H, W)]
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = torch.stack([(x - (W - 1) / 2) * px + sx, (y - (H - 1) / 2) * py + sy, torch.ones_like(x)], -1)
    return torch.nn.functional.normalize(d, dim=-1).reshape(-1, 3).contiguous()


def palette_of(N):
    g = torch.Generator().manual_seed(23)
    return (0.2 + 0.8 * torch.rand(N, 3, generator=g)).contiguous()


def background_of(H, W):
    g = torch.Generator().manual_seed(29)
    return torch.randint(0, 256, (H * W, 3), generator=g, dtype=torch.uint8)


def pointer(t):
    return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


OUTPUTS = ("converged_bits", "shadow_bits", "instance", "range", "colors", "positions", "normals")


def fresh_outputs(dev, H, W, skip=()):
    """Outputs filled with patterns no result equals."""
    rb = (W + 7) // 8
    out = dict(converged_bits=torch.full((H, rb), 0xA5, dtype=torch.uint8, device=dev), shadow_bits=torch.full((H, rb), 0xA5, dtype=torch.uint8, device=dev),
               instance=torch.full((H * W,), 0xA5, dtype=torch.uint8, device=dev), range=torch.full((H * W,), float("nan"), device=dev),
               colors=torch.full((H * W, 3), 0xA5, dtype=torch.uint8, device=dev), positions=torch.full((H * W, 3), float("nan"), device=dev),
               normals=torch.full((H * W, 3), float("nan"), device=dev))
    return {key: None if key in skip else value for key, value in out.items()}


def run_surface(dev, instances, H, W, cam, dirs, out, mlp=None, hard=True, light=None, palette=None, background=None, offset=None, alpha=1.0, shadows=True,
                header=None, frames=None, capacity=None, view=0, num_views=1, iterations=TRACE[0], background_pixels=None, temperature=T, config=True,
                surface=True):
    """One vsrd_frame_surface call -> its code.  Every pointer is a tensor, an address or None."""
    from vsrd_amd import _lib
    from vsrd_amd.rendering import renderers
    lib = _lib.load()
    N = int(instances.shape[0]) if capacity is None else capacity
    field = _lib.Field(N, temperature, None if instances is None else pointer(instances).value, None if mlp is None else pointer(mlp).value)
    render = _lib.make_config(0, 2, (0.0, 1.0), 1.0, 1.0, 1.0e-6, 3, frames=frames)
    cfg = renderers.surface_config(view, num_views, H, W, iterations, TRACE[1], TRACE[2], TRACE[1] if offset is None else offset, hard=hard, shadows=shadows,
                                   background=background is not None, alpha=alpha, **SHADING)
    if background_pixels is not None:
        cfg.background_pixels = background_pixels
    return lib.vsrd_frame_surface(field, render if config else None, cfg if surface else None, pointer(cam), pointer(dirs), pointer(light), pointer(palette),
                                  pointer(background), *[pointer(out[key]) for key in OUTPUTS], pointer(header), _lib.stream())


CASES = [(N, residual, size, hard) for N, residual in ((3, False), (3, True), (1, False)) for size in SIZES for hard in (True, False)]


@pytest.mark.parametrize("N, residual, size, hard", CASES, ids=[f"N{N}{'res' if r else 'box'}-{s[0]}x{s[1]}-{'hard' if h else 'soft'}" for N, r, s, h in CASES])
def test_every_link_against_the_composition(dev, N, residual, size, hard):
    from vsrd_amd import _lib, fields, frames, rendering
    lib = _lib.load()
    H, W = size
    R = H * W
    instances, mlp = instances_of(dev, N), mlp_of(dev, N) if residual else None
    cam, dirs = torch.tensor([CAMERA], device=dev), rays(N, H, W).to(dev)
    light, palette = torch.tensor(LIGHT, device=dev), palette_of(N).to(dev)
    out = fresh_outputs(dev, H, W)
    assert run_surface(dev, instances, H, W, cam, dirs, out, mlp=mlp, hard=hard, light=light, palette=palette) == 0
    torch.cuda.synchronize()
    field = _lib.Field(N, T, instances.data_ptr(), None if mlp is None else mlp.data_ptr())
    block = fields.FieldBlock(instances, T, mlp, None, hard)

    # ---- positions, converged: vsrd_sphere_trace on the same rays, bit for bit; the bit layout is frames.unpack_masks'
    positions, converged = torch.empty(R, 3, device=dev), torch.empty(R, dtype=torch.uint8, device=dev)
    _lib.check(lib.vsrd_sphere_trace(field, pointer(cam), 0, pointer(dirs), None, R, *TRACE, 0, 1 if hard else 0, pointer(positions), pointer(converged), _lib.stream()))
    torch.cuda.synchronize()
    converged = converged.bool()
    assert torch.equal(out["positions"], positions)
    mine = torch.from_numpy(frames.unpack_masks(out["converged_bits"].cpu().numpy()[None], W)[0]).to(dev).reshape(R)
    assert torch.equal(mine, converged)
    packed = np.packbits(converged.reshape(H, W).cpu().numpy(), axis=-1)
    assert np.array_equal(out["converged_bits"].cpu().numpy(), packed)                            # (pad bits 0: packbits pads with zeros)
    share = float(converged.float().mean())
    runs = [bool(converged.reshape(H, W)[y, x0:x0 + 64].any()) for y in range(H) for x0 in range(0, W, 64)]
    print(f"converged {int(converged.sum())} of {R}, empty runs {runs.count(False)} of {len(runs)}")
    assert 0.25 <= share <= 0.75 and runs.count(False) >= 1

    # ---- instance: the first arg-min over the single-member fields at the kernel's own positions
    members = torch.empty(N, R, device=dev)
    for n in range(N):
        one = _lib.Field(1, T, instances[n:n + 1].data_ptr(), None if mlp is None else mlp[n:n + 1].data_ptr())
        _lib.check(lib.vsrd_field_eval(one, pointer(positions), R, pointer(members[n]), None, None, 1, _lib.stream()))
    smallest = members == members.min(0).values
    first = (smallest * torch.arange(N, 0, -1, device=dev)[:, None]).argmax(0)                    # (distinct weights: the first minimum, whatever argmax does with ties)
    want_instance = torch.where(converged, first, torch.full_like(first, 255)).to(torch.uint8)
    assert torch.equal(out["instance"], want_instance)
    if N > 1:
        assert len(set(out["instance"][converged].tolist())) > 1

    # ---- normals: F.normalize of vsrd_field_eval's gradient at the kernel's own positions, every component within 4 spacings of 1
    gradients = torch.empty(R, 3, device=dev)
    _lib.check(lib.vsrd_field_eval(field, pointer(positions), R, None, pointer(gradients), None, 1 if hard else 0, _lib.stream()))
    want_normals = torch.nn.functional.normalize(gradients, dim=-1)
    error = (out["normals"] - want_normals).abs()[converged].max()
    print(f"max |normal - F.normalize(gradient)| = {float(error):.3e} (bound {4 * ULP:.3e})")
    assert error <= 4 * ULP
    assert (out["normals"][~converged].view(torch.int32) == 0).all()

    # ---- range: |position - origin| within 4 float32 spacings of the value
    want_range = (positions - cam[0]).norm(dim=-1)
    spacing = torch.nextafter(want_range, torch.full_like(want_range, float("inf"))) - want_range
    error = ((out["range"] - want_range).abs() / spacing)[converged].max()
    print(f"max |range - norm| = {float(error):.2f} spacings")
    assert error <= 4.0
    assert (out["range"][~converged].view(torch.int32) == 0).all()

    # ---- shadow: rendering.shadow_rendering fed the kernel's own positions, normals and converged, offset = criteria
    light_rays = light.expand(H, W, 3)
    shadow = rendering.shadow_rendering(block, out["positions"].view(H, W, 3), out["normals"].view(H, W, 3), light_rays, TRACE[0], TRACE[1],
                                        converged.view(H, W, 1), bounding_radius=TRACE[2]).reshape(R)
    mine = torch.from_numpy(frames.unpack_masks(out["shadow_bits"].cpu().numpy()[None], W)[0]).to(dev).reshape(R)
    print(f"shadowed {int(shadow.sum())}, lit {int((converged & ~shadow).sum())}")
    assert torch.equal(mine, shadow)
    assert np.array_equal(out["shadow_bits"].cpu().numpy(), np.packbits(shadow.reshape(H, W).cpu().numpy(), axis=-1))
    assert bool(shadow.any()) and bool((converged & ~shadow).any())
    # ... and offset = 2 criteria: the same trace started from positions + normals * 2c
    far = fresh_outputs(dev, H, W, skip=("colors",))
    assert run_surface(dev, instances, H, W, cam, dirs, far, mlp=mlp, hard=hard, light=light, offset=2 * TRACE[1]) == 0
    start = far["positions"].view(H, W, 3) + far["normals"].view(H, W, 3) * (2 * TRACE[1])
    _, hit = rendering.sphere_tracing(block, start, -light_rays, TRACE[0], TRACE[1], foreground_masks=converged.view(H, W, 1), bounding_radius=TRACE[2],
                                      initialization=False)
    want_far = (converged.view(H, W, 1) & hit).reshape(R)
    assert torch.equal(far["positions"], positions) and far["colors"] is None
    assert torch.equal(torch.from_numpy(frames.unpack_masks(far["shadow_bits"].cpu().numpy()[None], W)[0]).to(dev).reshape(R), want_far)
    assert bool(want_far.any()) and bool((converged & ~want_far).any())

    # ---- colours: phong_shading on the kernel's own normals and shadow, composed and quantised the same way, within 1 level
    def shaded(diffuse_light, specular_light):
        return rendering.phong_shading(dirs, out["normals"], light.expand(R, 3), torch.tensor(SHADING["light_ambient"], device=dev), diffuse_light, specular_light,
                                       torch.tensor(SHADING["material_ambient"], device=dev), palette[out["instance"].long().clamp(max=N - 1)],
                                       torch.tensor(SHADING["material_specular"], device=dev), torch.tensor(SHADING["material_emission"], device=dev),
                                       SHADING["shininess"])
    lit = shaded(torch.tensor(SHADING["light_diffuse"], device=dev), torch.tensor(SHADING["light_specular"], device=dev))
    dark = shaded(torch.zeros(3, device=dev), torch.zeros(3, device=dev))
    colour = torch.where(shadow[:, None], dark, lit)
    quantise = lambda c: (255.0 * c + 0.5).to(torch.int32)
    flat = quantise(torch.tensor(SHADING["background_color"], device=dev)).expand(R, 3)
    want = torch.where(converged[:, None], quantise(colour), flat)
    error = (out["colors"].to(torch.int32) - want).abs()
    print(f"max colour error {int(error.max())} levels, {int((error > 0).sum())} channels off")
    assert int(error[converged].max()) <= 1 and int(error[~converged].max()) == 0
    assert len(torch.unique(out["colors"][converged], dim=0)) >= 2                    # (a lit and a shadowed colour at the least)
    # ... and laid over a photograph: alpha c + (1 - alpha) background / 255; the background itself where nothing converged
    background, alpha = background_of(H, W).to(dev), 0.7
    over = fresh_outputs(dev, H, W)
    assert run_surface(dev, instances, H, W, cam, dirs, over, mlp=mlp, hard=hard, light=light, palette=palette, background=background, alpha=alpha) == 0
    want = torch.where(converged[:, None], quantise(alpha * colour + (1.0 - alpha) * background.float() / 255.0), background.to(torch.int32))
    error = (over["colors"].to(torch.int32) - want).abs()
    assert int(error[converged].max()) <= 1 and int(error[~converged].max()) == 0
    for key in ("converged_bits", "shadow_bits", "instance", "range", "positions", "normals"):
        assert torch.equal(over[key].view(torch.uint8), out[key].view(torch.uint8)), key


def arena_fields(cap, H, W, residual):
    from vsrd_amd import _lib
    f32, u8, rb = torch.float32, torch.uint8, (W + 7) // 8
    return ([("instances", (cap, 16), f32)] + ([("mlp", (cap, _lib.MLP_WEIGHTS), f32)] if residual else []) +
            [("cam", (1, 3), f32), ("dirs", (H * W, 3), f32), ("light", (3,), f32), ("palette", (cap, 3), f32), ("background", (H * W, 3), u8),
             ("header", (6,), torch.int32), ("converged_bits", (H, rb), u8), ("shadow_bits", (H, rb), u8), ("instance", (H * W,), u8), ("range", (H * W,), f32),
             ("colors", (H * W, 3), u8), ("positions", (H * W, 3), f32), ("normals", (H * W, 3), f32)])


@pytest.mark.parametrize("residual", [False, True], ids=["box", "residual"])
def test_batch_with_headers_equals_each_frame_alone(dev, residual):
    """Three frames in one arena with fill patterns between the buffers, capacity 4 with n_f = (4, 2, 3): each frame's outputs are, bit for
    bit, those of the one-frame call on that frame alone with its own N, and every byte outside the frames' outputs is untouched."""
    H, W, cap, counts = 6, 76, 4, (4, 2, 3)
    arena = RowArena(arena_fields(cap, H, W, residual), len(counts), 0x5A5A5A5A, 512)
    own = []
    for f, n in enumerate(counts):
        instances, mlp = instances_of(dev, n), mlp_of(dev, n, seed=40 + f) if residual else None
        instances[:, 0] += 0.3 * f
        frame = dict(instances=instances, mlp=mlp, cam=torch.tensor([CAMERA], device=dev), dirs=rays(n, H, W).to(dev), light=torch.tensor(LIGHT, device=dev) + 0.1 * f,
                     palette=palette_of(cap)[:n].contiguous().to(dev), background=background_of(H, W).to(dev) + f)
        arena.view("instances", f)[:n] = instances.cpu()
        if residual:
            arena.view("mlp", f)[:n] = mlp.cpu()
        for name in ("cam", "dirs", "light", "background"):
            arena.view(name, f).copy_(frame[name].cpu())
        arena.view("palette", f)[:n] = frame["palette"].cpu()
        arena.write_header(f, n)
        own.append(frame)
    device = arena.host.to(dev)
    at = arena.pointers(device, null=() if residual else ("mlp",))
    for hard in (True, False):
        device.copy_(arena.host)
        alone = []
        for frame in own:
            alone.append(fresh_outputs(dev, H, W))
            assert run_surface(dev, frame["instances"], H, W, frame["cam"], frame["dirs"], alone[-1], mlp=frame["mlp"], hard=hard, light=frame["light"],
                               palette=frame["palette"], background=frame["background"], alpha=0.6) == 0
        code = run_surface(dev, at("instances"), H, W, at("cam"), at("dirs"), {key: at(key) for key in OUTPUTS}, mlp=at("mlp") if residual else None, hard=hard,
                           light=at("light"), palette=at("palette"), background=at("background"), alpha=0.6, header=at("header"), frames=(len(counts), arena.stride),
                           capacity=cap)
        assert code == 0
        torch.cuda.synchronize()
        after = device.cpu()
        written = torch.zeros(arena.host.shape, dtype=torch.bool)
        for f, n in enumerate(counts):
            for key in OUTPUTS:
                offset, nbytes, _, _ = arena.layout[key]
                written[f * arena.stride + offset:f * arena.stride + offset + nbytes] = True
                assert torch.equal(arena.view(key, f, host=after).reshape(-1).view(torch.uint8), alone[f][key].cpu().reshape(-1).view(torch.uint8)), (hard, f, key)
            owners = arena.view("instance", f, host=after)
            assert 0 < int((owners != 255).sum()) < H * W and int(owners[owners != 255].max()) < n
        assert torch.equal(after[~written], arena.host[~written])


def test_eager_and_captured_replay_give_the_same_bytes(dev):
    N, (H, W) = 3, SIZES[0]
    instances, mlp = instances_of(dev, N), mlp_of(dev, N)
    cam, dirs = torch.tensor([CAMERA], device=dev), rays(N, H, W).to(dev)
    light, palette, background = torch.tensor(LIGHT, device=dev), palette_of(N).to(dev), background_of(H, W).to(dev)
    call = lambda out: run_surface(dev, instances, H, W, cam, dirs, out, mlp=mlp, hard=False, light=light, palette=palette, background=background, alpha=0.5)
    eager = [fresh_outputs(dev, H, W) for _ in range(2)]
    assert call(eager[0]) == 0 and call(eager[1]) == 0
    replayed = fresh_outputs(dev, H, W)
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.graph(graph, stream=stream):
        assert call(replayed) == 0
    for value in replayed.values():
        value.view(torch.uint8).fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    for key in OUTPUTS:
        assert torch.equal(eager[0][key].view(torch.uint8), eager[1][key].view(torch.uint8)), key
        assert torch.equal(eager[0][key].view(torch.uint8), replayed[key].view(torch.uint8)), key
    assert bool(eager[0]["converged_bits"].any())


def test_refusals_write_nothing(dev):
    """Every VSRD_E_INVALID_ARGUMENT case of the header; none launches anything: the arena is compared before and after."""
    from vsrd_amd import _lib
    N, (H, W) = 3, SIZES[1]
    arena = RowArena(arena_fields(N, H, W, False), 2, 0x3C3C3C3C, 256)
    arena.view("instances")[:] = instances_of(dev, N).cpu()
    arena.view("cam").copy_(torch.tensor([CAMERA]))
    arena.view("dirs").copy_(rays(N, H, W))
    arena.view("light").copy_(torch.tensor(LIGHT))
    arena.view("palette").copy_(palette_of(N))
    device = arena.host.to(dev)
    at = arena.pointers(device)
    good = dict(instances=at("instances"), H=H, W=W, cam=at("cam"), dirs=at("dirs"), out={key: at(key) for key in OUTPUTS}, light=at("light"), palette=at("palette"),
                capacity=N)
    without = lambda *names: {key: None if key in names else at(key) for key in OUTPUTS}
    bad = [dict(view=1), dict(view=-1), dict(view=2, num_views=2), dict(capacity=0), dict(capacity=_lib.MAX_INSTANCES + 1),
           dict(light=None), dict(light=None, alpha=1.0, shadows=False),                            # colours without a light: no shading was asked for
           dict(palette=None), dict(background=at("background"), background_pixels=0), dict(background=at("background"), background_pixels=H * W - 1),
           dict(instances=None), dict(cam=None), dict(dirs=None), dict(config=False), dict(surface=False), dict(H=0), dict(W=0), dict(iterations=-1),
           dict(temperature=0.0), dict(frames=(2, 100)), dict(num_views=0)]
    for change in bad:
        arguments = dict(good, **change)
        code = run_surface(dev, arguments.pop("instances"), arguments.pop("H"), arguments.pop("W"), arguments.pop("cam"), arguments.pop("dirs"),
                           arguments.pop("out"), **arguments)
        assert code == _lib.E_INVALID_ARGUMENT, change
    torch.cuda.synchronize()
    assert torch.equal(device.cpu(), arena.host)
    # ... and the same call without the change, without colours and a light, and with both frames, is served
    for change in (dict(), dict(light=None, palette=None, out=without("colors")), dict(frames=(2, arena.stride)), dict(out=without(*OUTPUTS))):
        arguments = dict(good, **change)
        assert run_surface(dev, arguments.pop("instances"), arguments.pop("H"), arguments.pop("W"), arguments.pop("cam"), arguments.pop("dirs"),
                           arguments.pop("out"), **arguments) == 0, change
    torch.cuda.synchronize()
    assert not torch.equal(device.cpu(), arena.host)


def test_frame_optimizer_and_frame_batch_surface(dev):
    """V = 3, 64 x 76, N = 4, 48 rays, two box-only and two residual steps: surface() of a batch row equals surface() of the frame in a slot of
    its own and rendering.surface_render on the row's field block; a loop that calls surface() between steps walks the trajectory of a twin
    that never does; surface() before any step raises."""
    from vsrd_amd import fields, launcher, optimization, rendering
    size, V, N = (64, 76), 3, 4
    inputs = [launcher.synthetic_frame_inputs(dev, 3, V, N, *size), launcher.synthetic_frame_inputs(dev, 4, V, 3, *size)]
    config = optimization.OptimizationConfig(num_samples=40, num_rays=48, warmup_steps=2, num_steps=12, seed=3, mlp_adjoint_item_slots=8,
                                             surface_num_iterations=64)
    g = torch.Generator().manual_seed(31)
    photographs = [torch.randint(0, 256, (*size, 3), generator=g, dtype=torch.uint8).to(dev) for _ in inputs]
    keys = ("converged_bits", "shadow_bits", "instance", "range", "colors")

    def parameters(loop):
        return [t.detach().clone() for t in (loop.detector.locations, loop.detector.dimensions, loop.detector.orientations, loop.detector.embeddings)]

    def start_at_the_truth(loop, k):
        """A loop starts with every box at (0, 0.675, 50) m, one pixel of this image, and four steps move it little: the loops of this test start
        from the boxes their frames were made of (synthetic.synthetic_frame), which cover 235 and 74 pixels (float64 oracle)."""
        from vsrd_amd import synthetic
        _, _, location, dimension, orientation = synthetic.synthetic_frame(3 + k, V, *size, loop.num_instances)
        with torch.no_grad():
            loop.detector.locations.copy_(location); loop.detector.dimensions.copy_(dimension); loop.detector.orientations.copy_(orientation)

    def snapshot(result):
        return {key: value.clone() if isinstance(value, torch.Tensor) else value for key, value in result.items()}
    alone, untouched = [], []
    for k, frame in enumerate(inputs):
        for asked in (True, False):
            loop = optimization.FrameOptimizer(frame, dataclasses.replace(config, init_seed=70 + k), dev, graph=True, persistent=True)
            start_at_the_truth(loop, k)
            shots = []
            if asked:
                with pytest.raises(RuntimeError, match="no step has run"):
                    loop.surface()
            for phase in range(2):                                   # after two box-only steps, after two residual steps
                loop.run(2, steps_per_graph=1)
                if asked:
                    shots.append(snapshot(loop.surface(background=photographs[k])))
                    shots.append(snapshot(loop.surface(hard=False, light=LIGHT)))
                    # ... against the eager one-frame entry on the row's field block
                    n, residual = loop.num_instances, phase == 1
                    block = fields.FieldBlock(loop._glue["instances"][:n].contiguous(), float(loop.schedule[0]),
                                              loop._glue["mlp_centred"][:n].contiguous() if residual else None, None, False)
                    eager = rendering.surface_render(block, loop.camera_positions[0], loop.ray_directions[:size[0] * size[1]].view(*size, 3),
                                                     config.surface_num_iterations, config.surface_convergence_criteria, config.surface_bounding_radius, light=LIGHT)
                    torch.cuda.synchronize()
                    for key in keys:
                        assert torch.equal(shots[-1][key], eager[key]), (k, phase, key)
                    assert 0 < int(np.unpackbits(eager["converged_bits"].cpu().numpy()).sum()) < size[0] * size[1]
            torch.cuda.synchronize()
            (alone if asked else untouched).append(shots if asked else parameters(loop))
            if asked:
                alone[-1] = (shots, parameters(loop))
            loop.close()
    for (shots, after), without in zip(alone, untouched):            # surface() leaves the trajectory bit-identical
        assert all(torch.equal(a, b) for a, b in zip(after, without))
    plain = optimization.FrameBatch(inputs, config, dev, init_seeds=[70, 71], max_instances=N)
    plain.run(1, steps_per_graph=1)
    with pytest.raises(RuntimeError, match="surface=True"):
        plain.surface()
    plain.close()
    batch = optimization.FrameBatch(inputs, config, dev, init_seeds=[70, 71], max_instances=N, surface=True)
    with pytest.raises(RuntimeError, match="no step has run"):
        batch.surface()
    for k, member in enumerate(batch.frames):
        start_at_the_truth(member, k)
    for phase in range(2):
        batch.run(2, steps_per_graph=1)
        for which, arguments in enumerate((dict(background=photographs), dict(hard=False, light=LIGHT))):
            got = batch.surface(**arguments)
            torch.cuda.synchronize()
            for k, mine in enumerate(got):
                want = alone[k][0][2 * phase + which]
                for key in keys:
                    assert torch.equal(mine[key], want[key]), (phase, which, k, key)
                assert mine["shape"] == size and int(mine["instance"][mine["instance"] != 255].max()) < inputs[k].soft_masks.shape[-1]
    torch.cuda.synchronize()
    for k, member in enumerate(batch.frames):
        assert all(torch.equal(a, b) for a, b in zip(parameters(member), untouched[k]))
    batch.close()
