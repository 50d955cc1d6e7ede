"""vsrd_frame_photometric_with_header, vsrd_frame_photometric_finish_with_header and vsrd_sample_rays_table_frames (include/vsrd_hip.h): the
photometric term, its finish and its draw for every frame of a batch in one call each.  The reference is today's one-frame symbol on each
frame alone -- vsrd_frame_photometric, vsrd_frame_photometric_finish, vsrd_sample_rays_table -- and everything here is equality of BITS:
there is no tolerance.

The frames lie in one arena, every buffer at the same offset of every row, the rows a multiple of 256 bytes apart; behind every buffer of
a row lie GAP bytes of a fill pattern (the last gap of a row is what separates it from the next row), and the whole arena is compared
against its expected contents, so a write outside a frame's own buffers shows.

The scene is tests/test_hip_frame_photometric.py's "residual-48" at the size a batch test needs: V = 3 (capacity 4 in the mixed case),
128 x 128, N <= 4, 48 rays, 100 trace iterations, 11 x 11 patches, top_k = 3.  The frames differ in box parameters, MLP weights and images.
"""
import ctypes
import functools

import pytest
import torch

import patch_correlation_reference as pcr
from test_hip_frame_photometric import CRITERION, ITERATIONS, RADIUS, SCALE, T, same_bits

pytestmark = pytest.mark.gpu

H, W, PATCH, TOP_K, R = 128, 128, (11, 11), 3, 48
GAP, FILL = 256, 0x5B
FRAMES = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


# ---- the frames ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame_scene(frame, N, V, residual):
    """Host tensors of one frame: cameras, images, N boxes (and MLP weights), the pixel indices of its R rays."""
    generator = torch.Generator().manual_seed(700 + frame)
    K, E = pcr.cameras(V, H, W)
    images = pcr.smooth_images(generator, V, H, W)
    locations = torch.tensor([[-2.0, 0.6, 14.0], [0.5, 0.5, 18.0], [2.5, 0.7, 12.0], [-0.8, 0.55, 10.0]])[:N] + 0.15 * frame
    dimensions = torch.tensor([[0.9, 0.8, 2.0], [0.9, 0.8, 2.0], [0.8, 0.75, 1.8], [0.7, 0.7, 1.6]])[:N]
    yaws = torch.tensor([0.3, -0.5, 1.1, 0.8])[:N] + 0.2 * frame
    rotations = torch.stack([torch.stack([torch.cos(yaws), torch.zeros(N), torch.sin(yaws)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                             torch.stack([-torch.sin(yaws), torch.zeros(N), torch.cos(yaws)], -1)], -2)
    aims = locations[torch.arange(R) % N] + torch.randn(R, 3, generator=generator) * torch.tensor([0.5, 0.4, 0.5])
    projected = aims @ K[0].T
    pixels = (projected[:, :2] / projected[:, 2:]).round().long()
    pixels[:, 0].clamp_(12, W - 13); pixels[:, 1].clamp_(12, H - 13)
    mlp = torch.randn(N, 1617, generator=generator) * 0.05 if residual else None
    return dict(K=K, E=E, images=images, locations=locations, dimensions=dimensions, rotations=rotations, indices=pixels[:, 1] * W + pixels[:, 0], mlp=mlp)


_frames = {}


def frame_on_device(dev, frame, N, V, residual, away=False):
    """The frame's device tensors as a one-frame call takes them (away: the ray directions negated, so that every ray leaves through the
    bounding radius)."""
    key = (frame, N, V, residual, away)
    if key not in _frames:
        from vsrd_amd import fields, losses, rendering
        from vsrd_amd.rendering import renderers
        s = frame_scene(frame, N, V, residual)
        K, E = s["K"].to(dev), s["E"].to(dev)
        cam, dirs = rendering.ray_casting((H, W), K, E)
        directions = dirs[0].reshape(-1, 3).contiguous()
        _frames[key] = dict(
            K=K.contiguous(), E=E.contiguous(), gray=losses.grayscale_images(s["images"].to(dev)).contiguous(), camera=cam[0].contiguous(),
            directions=-directions if away else directions, indices=s["indices"].to(dev),
            instances=fields.pack_instances(s["locations"], s["rotations"], s["dimensions"]).to(dev).contiguous(),
            mlp=None if s["mlp"] is None else renderers._centre_mlp(s["mlp"].to(dev).contiguous()).contiguous())
    return _frames[key]


def pattern(rows, columns, dev, frame=0):
    """A known pattern with both zeros' signs in it (tests/test_hip_frame_photometric.py), another one for every frame."""
    values = torch.arange(rows * columns, dtype=torch.float32) / 7.0 - 3.0 + 0.25 * frame
    values[::5] = 0.0
    values[::11] = -0.0
    return values.view(rows, columns).to(dev)


# ---- the arena ----------------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("loss", "stats", "own_instances", "own_mlp", "grad_instances", "grad_mlp", "positions", "normals", "converged")


class Batch:
    """B frames in one arena, laid out for the capacities (N, V), and the calls on it.  `counts`: per frame (n_f, v_f) or None: uniform.
    Every frame's inputs sit in the leading n_f instances / v_f views of its buffers, the rest of every buffer is NaN (inputs) or the
    fill the outputs start from."""

    def __init__(self, dev, frames, N, V, residual, counts=None, away=()):
        from vsrd_amd import _lib
        self.lib, self.dev, self.N, self.V, self.residual, self.B = _lib.load(), dev, N, V, residual, len(frames)
        self.counts = counts or [(N, V)] * self.B
        self.alone = [frame_on_device(dev, f, n, v, residual, away=(f in away)) for f, (n, v) in zip(frames, self.counts)]
        self.workspace_bytes = self.lib.vsrd_frame_photometric_workspace_bytes(N, 1 if residual else 0, V, R, PATCH[0] * PATCH[1])
        assert self.workspace_bytes > 0
        f32, u8, i64 = torch.float32, torch.uint8, torch.int64
        spec = [("camera", (3,), f32), ("directions", (H * W, 3), f32), ("gray", (V, H, W), f32), ("K", (V, 3, 3), f32), ("E", (V, 4, 4), f32),
                ("indices", (R,), i64), ("instances", (N, 16), f32), ("mlp", (N, 1617), f32), ("header", (24,), u8),
                ("workspace", (self.workspace_bytes,), u8), ("loss", (1,), f32), ("stats", (2,), f32), ("own_instances", (N, 16), f32),
                ("own_mlp", (N, 1617), f32), ("grad_instances", (N, 16), f32), ("grad_mlp", (N, 1617), f32), ("positions", (R, 3), f32),
                ("normals", (R, 3), f32), ("converged", (R,), u8), ("record", (5,), f32)]
        self.offsets, at = {}, 0
        for name, shape, dtype in spec:
            count = 1
            for x in shape:
                count *= x
            nbytes = count * torch.empty((), dtype=dtype).element_size()
            self.offsets[name] = (at, nbytes, shape, dtype)
            at = (at + nbytes + GAP + 255) & ~255
        self.stride = at
        whole = torch.full((self.B * self.stride + 256,), FILL, dtype=u8, device=dev)
        self.arena = whole[(-whole.data_ptr()) % 256:][:self.B * self.stride]
        nan = float("nan")
        for f, (d, (n, v)) in enumerate(zip(self.alone, self.counts)):
            self.view("camera", f).copy_(d["camera"]); self.view("directions", f).copy_(d["directions"]); self.view("indices", f).copy_(d["indices"])
            for name, rows in (("gray", v), ("K", v), ("E", v), ("instances", n)):
                self.view(name, f).fill_(nan)
                self.view(name, f)[:rows].copy_(d[name])
            self.view("mlp", f).fill_(nan)
            if residual:
                self.view("mlp", f)[:n].copy_(d["mlp"])
            header = _lib.FrameHeader(n | _lib.FRAME_HEADER_HAS_VIEWS, 1.0, v, 0, 0)
            self.view("header", f).copy_(torch.frombuffer(bytearray(bytes(header)), dtype=u8).to(dev))
            for name in ("loss", "stats", "own_instances", "own_mlp", "positions", "normals"):
                self.view(name, f).fill_(nan)
            self.view("converged", f).fill_(77)
            self.view("grad_instances", f).copy_(pattern(N, 16, dev, f)); self.view("grad_mlp", f).copy_(pattern(N, 1617, dev, f))
            self.view("record", f).copy_(torch.tensor([0.1, 0.2, 0.3, 0.4, 1.7 + f], device=dev))
        self.before = self.arena.clone()
        self.patch = _lib.PatchCorrelationConfig(V, R, H, W, PATCH[0], PATCH[1], TOP_K, 0, 1.0e-6, 1.0e-12)
        self.config = _lib.FramePhotometricConfig(ITERATIONS, CRITERION, RADIUS, SCALE, self.B, self.stride)

    def view(self, name, frame, arena=None):
        at, nbytes, shape, dtype = self.offsets[name]
        arena = self.arena if arena is None else arena
        return arena[frame * self.stride + at:frame * self.stride + at + nbytes].view(dtype).view(shape)

    def address(self, name):
        return self.arena.data_ptr() + self.offsets[name][0]

    def refill(self):
        self.arena.copy_(self.before)

    def __call__(self, header=False, symbol="vsrd_frame_photometric_with_header", **replace):
        from vsrd_amd import _lib
        field = _lib.Field(self.N, T, self.address("instances"), self.address("mlp") if self.residual else None)
        arguments = dict(config=self.config, patch=self.patch, field=field, camera=self.address("camera"), directions=self.address("directions"),
                         gray=self.address("gray"), intrinsics=self.address("K"), extrinsics=self.address("E"), indices=self.address("indices"),
                         workspace=self.address("workspace"), workspace_bytes=self.workspace_bytes, loss=self.address("loss"), stats=self.address("stats"),
                         own_instances=self.address("own_instances"), own_mlp=self.address("own_mlp"), grad_instances=self.address("grad_instances"),
                         grad_mlp=self.address("grad_mlp"), positions=self.address("positions"), normals=self.address("normals"),
                         converged=self.address("converged"))
        if symbol == "vsrd_frame_photometric_with_header":
            arguments["frame_header"] = self.address("header") if header else None
        arguments["stream"] = _lib.stream()
        arguments.update(replace)
        return getattr(self.lib, symbol)(*arguments.values())

    def expected(self, references):
        """The arena as it must be after the call: its contents of before with every frame's outputs replaced, in the leading n_f rows of
        the per-instance ones, by the one-frame call's.  The workspace is the call's own and is not compared."""
        want = self.before.clone()
        for f, (reference, (n, _)) in enumerate(zip(references, self.counts)):
            for name in OUTPUTS:
                if name in ("own_mlp", "grad_mlp") and not self.residual:
                    continue
                target = self.view(name, f, want)
                rows = n if name in ("own_instances", "own_mlp", "grad_instances", "grad_mlp") else target.shape[0]
                target[:rows].copy_(reference[name])
        return want

    def compare(self, references):
        """Every byte of the arena outside the workspaces against `expected`; -> the names of the buffers that differ, per frame."""
        want, wrong = self.expected(references), []
        at, nbytes = self.offsets["workspace"][:2]
        for f in range(self.B):
            got_row, want_row = self.arena[f * self.stride:(f + 1) * self.stride].clone(), want[f * self.stride:(f + 1) * self.stride]
            got_row[at:at + nbytes] = want_row[at:at + nbytes]
            if torch.equal(got_row, want_row):
                continue
            for name, (start, size, _, _) in self.offsets.items():
                if name != "workspace" and not torch.equal(got_row[start:start + size + GAP], want_row[start:start + size + GAP]):
                    wrong.append((f, name))
        return wrong


def alone(dev, d, frame=0):
    """Today's vsrd_frame_photometric on one frame's own tensors (laid out for its own n_f and v_f) -> its outputs."""
    from vsrd_amd import _lib
    lib = _lib.load()
    N, V, residual = d["instances"].shape[0], d["K"].shape[0], d["mlp"] is not None
    nan = float("nan")
    out = dict(loss=torch.full((1,), nan, device=dev), stats=torch.full((2,), nan, device=dev), own_instances=torch.full((N, 16), nan, device=dev),
               own_mlp=torch.full((N, 1617), nan, device=dev), grad_instances=pattern(4, 16, dev, frame)[:N].contiguous(),
               grad_mlp=pattern(4, 1617, dev, frame)[:N].contiguous(), positions=torch.full((R, 3), nan, device=dev),
               normals=torch.full((R, 3), nan, device=dev), converged=torch.full((R,), 77, dtype=torch.uint8, device=dev))
    nbytes = lib.vsrd_frame_photometric_workspace_bytes(N, 1 if residual else 0, V, R, PATCH[0] * PATCH[1])
    workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    patch = _lib.PatchCorrelationConfig(V, R, H, W, PATCH[0], PATCH[1], TOP_K, 0, 1.0e-6, 1.0e-12)
    config = _lib.FramePhotometricConfig(ITERATIONS, CRITERION, RADIUS, SCALE, 1, 0)
    _lib.check(lib.vsrd_frame_photometric(
        config, patch, _lib.make_field(d["instances"], T, d["mlp"]), _lib.ptr(d["camera"]), _lib.ptr(d["directions"]), _lib.ptr(d["gray"]), _lib.ptr(d["K"]),
        _lib.ptr(d["E"]), d["indices"].data_ptr(), workspace.data_ptr() + (-workspace.data_ptr()) % 256, nbytes, _lib.ptr(out["loss"]), _lib.ptr(out["stats"]),
        _lib.ptr(out["own_instances"]), _lib.ptr(out["own_mlp"]), _lib.ptr(out["grad_instances"]), _lib.ptr(out["grad_mlp"]), _lib.ptr(out["positions"]),
        _lib.ptr(out["normals"]), out["converged"].data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    return out


# ---- 1: a uniform batch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [True, False], ids=["residual", "box-only"])
def test_a_uniform_batch_equals_its_frames_alone(dev, residual):
    from vsrd_amd import _lib
    batch = Batch(dev, range(FRAMES), 3, 3, residual)
    assert batch.stride % 256 == 0
    _lib.check(batch(header=False))
    torch.cuda.synchronize()
    references = [alone(dev, d, f) for f, d in enumerate(batch.alone)]
    for f, reference in enumerate(references):
        assert int(reference["converged"].sum()) >= 1 and float(reference["stats"][1]) > 0, f
        assert not torch.isnan(reference["own_instances"]).any() and float(reference["own_instances"].abs().max()) > 0, f
    assert not same_bits(references[0]["loss"], references[1]["loss"]) and not same_bits(references[1]["loss"], references[2]["loss"])
    assert batch.compare(references) == []


# ---- 2: a frame without a converged ray among frames that have some -------------------------------------------------------------------------
def test_a_frame_without_a_converged_ray(dev):
    from vsrd_amd import _lib
    batch = Batch(dev, range(FRAMES), 3, 3, True, away=(1,))
    _lib.check(batch(header=False))
    torch.cuda.synchronize()
    references = [alone(dev, d, f) for f, d in enumerate(batch.alone)]
    converged = [int(batch.view("converged", f).sum()) for f in range(FRAMES)]
    assert converged[1] == 0 and converged[0] >= 1 and converged[2] >= 1, converged
    assert batch.compare(references) == []
    # the middle frame: its totals keep their bits, its own gradients are zero
    for name in ("grad_instances", "grad_mlp"):
        assert same_bits(batch.view(name, 1), batch.view(name, 1, batch.before)), name
    for name in ("own_instances", "own_mlp"):
        assert same_bits(batch.view(name, 1), torch.zeros_like(batch.view(name, 1))), name
    assert same_bits(batch.view("loss", 1), torch.zeros(1, device=dev)) and same_bits(batch.view("stats", 1), torch.zeros(2, device=dev))


# ---- 3: frames that differ in instance and view count ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [True, False], ids=["residual", "box-only"])
def test_mixed_counts(dev, residual):
    from vsrd_amd import _lib
    counts = [(4, 4), (2, 3), (3, 4)]
    batch = Batch(dev, range(FRAMES), 4, 4, residual, counts=counts)
    _lib.check(batch(header=True))
    torch.cuda.synchronize()
    references = [alone(dev, d, f) for f, d in enumerate(batch.alone)]
    for f, reference in enumerate(references):
        assert float(reference["stats"][1]) > 0, f
    # (compare holds every byte outside the frames' own n_f rows to the fill the arena started from: instances n_f .. N-1 are untouched,
    #  and the NaNs in instances n_f .. and views v_f .. of the inputs would show in the results had they been read)
    assert batch.compare(references) == []
    for f, (n, _) in enumerate(counts):
        for name in ("own_instances", "grad_instances") + (("own_mlp", "grad_mlp") if residual else ()):
            assert same_bits(batch.view(name, f)[n:], batch.view(name, f, batch.before)[n:]), (f, name)


def test_a_frame_with_fewer_views_than_top_k(dev):
    """top_k > v_f cannot be refused by the host side of the call: the frame is treated as one without a converged ray."""
    from vsrd_amd import _lib
    batch = Batch(dev, range(2), 3, 4, True, counts=[(3, 4), (3, 2)])
    _lib.check(batch(header=True))
    torch.cuda.synchronize()
    first = alone(dev, batch.alone[0], 0)
    assert float(first["stats"][1]) > 0
    for name in OUTPUTS:
        assert same_bits(batch.view(name, 0), first[name]), name
    assert same_bits(batch.view("loss", 1), torch.zeros(1, device=dev)) and same_bits(batch.view("stats", 1), torch.zeros(2, device=dev))
    for name in ("own_instances", "own_mlp"):
        assert same_bits(batch.view(name, 1), torch.zeros_like(batch.view(name, 1))), name
    for name in ("grad_instances", "grad_mlp"):
        assert same_bits(batch.view(name, 1), batch.view(name, 1, batch.before)), name


# ---- 4: the draw, the finish, capture and replay --------------------------------------------------------------------------------------------
def test_the_batched_draw_equals_the_frames_draws(dev):
    from vsrd_amd import _lib
    lib = _lib.load()
    count, samples, seed = H * W, R, 1234 + 2
    table_bytes = lib.vsrd_ray_table_bytes(count)
    step_at = (table_bytes + GAP + 255) & ~255                   # a row: the table | the step counter | the indices, gaps in between
    indices_at = step_at + 256
    stride = (indices_at + samples * 8 + GAP + 255) & ~255
    whole = torch.full((FRAMES * stride + 256,), FILL, dtype=torch.uint8, device=dev)
    arena = whole[(-whole.data_ptr()) % 256:][:FRAMES * stride]
    generator = torch.Generator().manual_seed(5)
    steps = [3, 250, 17]
    for f in range(FRAMES):
        weights = (torch.rand(count, generator=generator) * (torch.rand(count, generator=generator) < 0.4)).to(dev)
        _lib.check(lib.vsrd_ray_table_build(_lib.ptr(weights), count, arena.data_ptr() + f * stride, table_bytes, _lib.stream()))
        arena[f * stride + step_at:f * stride + step_at + 8].view(torch.int64).fill_(steps[f])
    torch.cuda.synchronize()
    want = []
    for f in range(FRAMES):
        indices = torch.full((samples,), -7, dtype=torch.int64, device=dev)
        _lib.check(lib.vsrd_sample_rays_table(arena.data_ptr() + f * stride, count, samples, seed, 0, arena.data_ptr() + f * stride + step_at, None,
                                              indices.data_ptr(), _lib.stream()))
        want.append(indices)
    torch.cuda.synchronize()
    before = arena.clone()
    _lib.check(lib.vsrd_sample_rays_table_frames(arena.data_ptr(), count, samples, seed, arena.data_ptr() + step_at, arena.data_ptr() + indices_at, FRAMES,
                                                 stride, _lib.stream()))
    torch.cuda.synchronize()
    expected = before.clone()
    for f in range(FRAMES):
        got = arena[f * stride + indices_at:f * stride + indices_at + samples * 8].view(torch.int64)
        assert torch.equal(got, want[f]), f
        assert int(got.min()) >= 0 and got.unique().numel() == samples
        expected[f * stride + indices_at:f * stride + indices_at + samples * 8].view(torch.int64).copy_(want[f])
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    assert torch.equal(arena, expected)                          # tables, counters and the gaps between the rows as they were
    for bad in ((FRAMES, 100), (FRAMES, 0), (1025, stride)):
        assert lib.vsrd_sample_rays_table_frames(arena.data_ptr(), count, samples, seed, arena.data_ptr() + step_at, arena.data_ptr() + indices_at, *bad,
                                                 _lib.stream()) == _lib.E_INVALID_ARGUMENT
    assert lib.vsrd_sample_rays_table_frames(arena.data_ptr(), count, samples, seed, None, arena.data_ptr() + indices_at, FRAMES, stride,
                                             _lib.stream()) == _lib.E_INVALID_ARGUMENT


def test_the_batched_finish_equals_the_frames_finishes(dev):
    from vsrd_amd import _lib
    batch = Batch(dev, range(FRAMES), 3, 3, False, away=(1,))
    _lib.check(batch(header=False))
    torch.cuda.synchronize()
    weight = 0.05
    want = []
    for f in range(FRAMES):
        record = batch.view("record", f).clone()
        _lib.check(batch.lib.vsrd_frame_photometric_finish(_lib.ptr(batch.view("loss", f)), _lib.ptr(batch.view("stats", f)), weight, _lib.ptr(record),
                                                           _lib.stream()))
        want.append(record)
    torch.cuda.synchronize()
    kept = batch.arena.clone()
    _lib.check(batch.lib.vsrd_frame_photometric_finish_with_header(batch.address("loss"), batch.address("stats"), weight, batch.address("record"), FRAMES,
                                                                   batch.stride, _lib.stream()))
    torch.cuda.synchronize()
    for f in range(FRAMES):
        assert same_bits(batch.view("record", f), want[f]), f
        batch.view("record", f, kept).copy_(want[f])
    assert same_bits(batch.view("record", 1), batch.view("record", 1, batch.before))         # no converged ray: the record keeps its bits
    assert not same_bits(batch.view("record", 0), batch.view("record", 0, batch.before))
    assert torch.equal(batch.arena, kept)
    assert batch.lib.vsrd_frame_photometric_finish_with_header(batch.address("loss"), batch.address("stats"), weight, batch.address("record"), FRAMES, 100,
                                                               _lib.stream()) == _lib.E_INVALID_ARGUMENT
    assert batch.lib.vsrd_frame_photometric_finish_with_header(None, batch.address("stats"), weight, batch.address("record"), FRAMES, batch.stride,
                                                               _lib.stream()) == _lib.E_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.equal(batch.arena, kept)


def test_two_calls_and_a_replay_give_the_same_bits(dev):
    from vsrd_amd import _lib
    batch = Batch(dev, range(FRAMES), 4, 4, True, counts=[(4, 4), (2, 3), (3, 4)])
    at, nbytes = batch.offsets["workspace"][:2]

    def snapshot():
        result = batch.arena.clone()
        for f in range(FRAMES):
            result[f * batch.stride + at:f * batch.stride + at + nbytes] = 0
        return result
    results = []
    for _ in range(2):
        batch.refill()
        _lib.check(batch(header=True))
        torch.cuda.synchronize()
        results.append(snapshot())
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.graph(graph, stream=stream):
        batch.refill()
        _lib.check(batch(header=True))
    batch.arena.fill_(3)                                         # (the replay's own refill puts the start values back)
    graph.replay()
    torch.cuda.synchronize()
    results.append(snapshot())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])
    assert all(float(batch.view("stats", f)[1]) > 0 for f in range(FRAMES))


# ---- 5: refusals write nothing --------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    from vsrd_amd import _lib
    batch = Batch(dev, range(FRAMES), 3, 3, True)

    def config(num_frames, stride, iterations=ITERATIONS):
        return _lib.FramePhotometricConfig(iterations, CRITERION, RADIUS, SCALE, num_frames, stride)
    invalid = [("stride no multiple of 256", batch(config=config(FRAMES, batch.stride + 4))), ("stride 0", batch(config=config(FRAMES, 0))),
               ("negative stride", batch(config=config(FRAMES, -batch.stride))), ("too many frames", batch(config=config(1025, batch.stride))),
               ("negative iterations", batch(config=config(FRAMES, batch.stride, -1)))]
    for name in ("config", "patch", "field", "camera", "directions", "gray", "intrinsics", "extrinsics", "indices", "loss", "stats", "own_instances",
                 "own_mlp", "grad_instances", "grad_mlp"):
        invalid.append((name, batch(**{name: None})))
    invalid.append(("top_k beyond the view capacity", batch(patch=_lib.PatchCorrelationConfig(3, R, H, W, PATCH[0], PATCH[1], 4, 0, 1.0e-6, 1.0e-12))))
    invalid.append(("too many rays", batch(patch=_lib.PatchCorrelationConfig(3, 2049, H, W, PATCH[0], PATCH[1], TOP_K, 0, 1.0e-6, 1.0e-12))))
    invalid.append(("a workspace off its alignment", batch(workspace=batch.address("workspace") + 4)))
    for name, code in invalid:
        assert code == _lib.E_INVALID_ARGUMENT, (name, code)
    assert batch(workspace=None) == _lib.E_WORKSPACE and batch(workspace_bytes=batch.workspace_bytes - 1) == _lib.E_WORKSPACE
    # the one-frame symbol keeps its contract: a batch is unsupported there
    assert batch(symbol="vsrd_frame_photometric") == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(batch.arena, batch.before)
    # the call still works after all that
    _lib.check(batch())
    torch.cuda.synchronize()
    assert not torch.equal(batch.arena, batch.before)
    assert batch.compare([alone(dev, d, f) for f, d in enumerate(batch.alone)]) == []
