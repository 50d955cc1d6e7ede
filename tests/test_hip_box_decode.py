"""models.BoxParameters3D on the library's two decode kernels (csrc/box_decode.h: vsrd_box_decode_forward / _backward) against the module's
eager torch path on the same device, against float64 autograd on the CPU, and the module-level behaviour around it (the dict, state_dict,
gradient accumulation, which modules leave the library alone).  The refusals are met without a device; everything else needs a real
MI355X: ``-m gpu``.

The kernels repeat torch's arithmetic op for op: every forward output and the raw gradients of a cotangent on the packed block alone (the
benchmark's case) come out bit for bit.  With cotangents on all five outputs the corners' part goes through torch's batched matmul and its
sums over the eight corners, whose orders the kernel does not repeat; there the bound below is four times the worst difference measured
against the eager path over this file's own cases, rounded up to one digit (docs/OPTLOG.md has the table).  0.0 means the values are equal."""
import pytest
import torch

from conftest import margin

DUMMY = 4096                     # a made-up non-null address: a refused call reads nothing behind it

# worst |native - eager| over the cases of this file, relative to the eager tensor's largest entry, times four and rounded up to one digit
# (measured "all": locations 2.355e-07 at [1-4], dimensions 1.934e-07 at [16-None], orientations 1.723e-06 at [1-None]; everything else 0)
FORWARD_BOUND = {"block": 0.0, "locations": 0.0, "dimensions": 0.0, "orientations": 0.0, "boxes_3d": 0.0}
BACKWARD_BOUND = {"block": {"locations": 0.0, "dimensions": 0.0, "orientations": 0.0},
                  "all": {"locations": 1e-6, "dimensions": 8e-7, "orientations": 7e-6}}

# (N, the special row of a one-box module or None: every special row)
CASES = [(1, None), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (5, None), (16, None), (64, None)]
NAMES = ("locations", "dimensions", "orientations")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def raw_parameters(N, special):
    """Raw parameters ~ N(0, 1) and, from row 0 on (one-box modules: row `special` of the list alone), the rows where the decode can go
    wrong: saturated sigmoids on both sides (exp(-x) overflows at x = -90), the normalize clamp -- a heading of (1e-20, 0), whose squared
    norm is subnormal, and of (0, 0) -- and a heading with cos exactly 0."""
    g = torch.Generator().manual_seed(1000 + 7 * N + (0 if special is None else special + 1))
    loc, dim, ori = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g), torch.randn(N, 2, generator=g)
    rows = [dict(loc=[20.0, -20.0, 90.0], dim=[-90.0, 20.0, -20.0]), dict(ori=[1.0e-20, 0.0]), dict(ori=[0.0, 0.0]), dict(ori=[0.0, -3.0]),
            dict(loc=[-90.0, 90.0, 0.0], dim=[90.0, -90.0, 0.0])]
    chosen = list(enumerate(rows)) if N >= len(rows) else ([] if special is None else [(0, rows[special])])
    for row, values in chosen:
        for name, tensor in (("loc", loc), ("dim", dim), ("ori", ori)):
            if name in values:
                tensor[row] = torch.tensor(values[name])
    return loc, dim, ori


def module(device, raws, dtype=torch.float32):
    from vsrd_amd import models
    m = models.BoxParameters3D(1, raws[0].shape[0])
    with torch.no_grad():
        m.locations.copy_(raws[0]); m.dimensions.copy_(raws[1]); m.orientations.copy_(raws[2])
    return m.to(device=device, dtype=dtype)


def eager_forward(m):
    """The module's torch ops, whatever device it is on (what forward() runs wherever the native path does not apply)."""
    from vsrd_amd import fields
    locations, dimensions = m.decode_location(m.locations), m.decode_dimension(m.dimensions)
    orientations = m.decode_orientation(m.orientations)
    out = dict(boxes_3d=m.decode_box_3d(locations, dimensions, orientations), locations=locations, dimensions=dimensions, orientations=orientations)
    n = locations.shape[1]
    out["block"] = torch.cat([locations[0].reshape(n, 3), orientations[0].reshape(n, 9), dimensions[0].reshape(n, 3), locations.new_zeros(n, 1)], dim=-1)
    if locations.dtype == torch.float32:             # (pack_instances hands out float32 whatever it is given)
        assert torch.equal(out["block"], fields.pack_instances(locations[0], orientations[0], dimensions[0]))
    return out


def native_forward(m):
    from vsrd_amd import fields
    out = dict(m())
    out["block"] = fields.pack_instances(out["locations"][0], out["orientations"][0], out["dimensions"][0])
    return out


def relative(a, b):
    """max |a - b| over max |b| (0 where both are all zero)."""
    scale = float(b.abs().max())
    return float((a.double() - b.double()).abs().max()) / scale if scale > 0 else float((a.double() - b.double()).abs().max())


def cotangents(out, which, seed):
    g = torch.Generator().manual_seed(seed)
    keys = ("block",) if which == "block" else ("block", "locations", "dimensions", "orientations", "boxes_3d")
    return {k: torch.randn(out[k].shape, generator=g).to(out[k].device, out[k].dtype) for k in keys}


def raw_gradients(m, out, grads):
    for p in (m.locations, m.dimensions, m.orientations):
        p.grad = None
    torch.autograd.backward([out[k] for k in grads], [grads[k] for k in grads])
    return {name: getattr(m, name).grad.detach().clone() for name in NAMES}


@pytest.mark.gpu
@pytest.mark.parametrize("N,special", CASES)
def test_forward_matches_the_eager_module(dev, N, special):
    """Every output and the packed block against the eager ops on the same device; the block IS what pack_instances hands the renderer (no
    cat is launched: the same storage comes back); the rotation rows carry exact 0 and 1."""
    m = module(dev, raw_parameters(N, special))
    native, eager = native_forward(m), eager_forward(m)
    tag = f"test_forward_matches_the_eager_module[{N}-{special}]"
    errors = {}
    for key, bound in FORWARD_BOUND.items():
        assert native[key].shape == eager[key].shape and native[key].dtype == eager[key].dtype and native[key].is_contiguous()
        errors[key] = margin(tag, key + " vs eager", relative(native[key], eager[key]), bound if bound > 0 else 1e-30)
        print(f"{tag}: {key}: max |native - eager| / max |eager| = {errors[key]:.3e}")
    assert all(errors[key] <= bound for key, bound in FORWARD_BOUND.items()), errors
    assert native["block"].shape == (N, 16) and torch.isfinite(native["block"]).all()
    assert torch.equal(native["block"][:, [4, 6, 7, 8, 10, 15]], torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev).expand(N, 6))
    assert torch.equal(native["block"][:, 3], native["block"][:, 11]) and torch.equal(native["block"][:, 5], -native["block"][:, 9])
    from vsrd_amd import fields
    out = m()
    again = fields.pack_instances(out["locations"][0], out["orientations"][0], out["dimensions"][0])
    assert again.grad_fn is not None and again.grad_fn is out["locations"].grad_fn          # the decode's own output, not a cat of views
    other = m()           # the outputs of two forwards mixed: a cat of what it is given, as before
    mixed = fields.pack_instances(out["locations"][0], other["orientations"][0], out["dimensions"][0])
    assert mixed.grad_fn is not again.grad_fn and mixed.data_ptr() != again.data_ptr() and torch.equal(mixed, again)


def three_ways(dev, N, special, which):
    """The raw gradients of one case: native, eager float32 on the device, float64 autograd on the CPU."""
    raws = raw_parameters(N, special)
    m = module(dev, raws)
    native_out = native_forward(m)
    grads = cotangents(native_out, which, 77 + N)
    native = raw_gradients(m, native_out, grads)
    eager = raw_gradients(m, eager_forward(m), grads)
    reference_module = module("cpu", raws, torch.float64)
    reference = raw_gradients(reference_module, eager_forward(reference_module), {k: v.double().cpu() for k, v in grads.items()})
    return native, eager, reference


@pytest.fixture(scope="module")
def eager_float64_error(dev):
    """The error the eager float32 path keeps against float64 autograd over this file's inputs: per cotangent set and parameter, the
    largest over the modules that hold every row of raw_parameters (N = 5, 16, 64), relative to the float64 gradient's largest entry.
    (A one-box module's gradient is two or three numbers, which the eager path now and then gets right to a tenth of an ulp; its own error
    is no bound anybody keeps.)  Measured: block 1.2e-07 / 1.0e-07 / 4.0e-08, all 1.1e-07 / 1.3e-07 / 1.3e-07 (locations / dimensions /
    orientations)."""
    worst = {which: dict.fromkeys(NAMES, 0.0) for which in ("block", "all")}
    for which in worst:
        for N, special in CASES:
            if N >= 5:
                _, eager, reference = three_ways(dev, N, special, which)
                for name in NAMES:
                    worst[which][name] = max(worst[which][name], relative(eager[name].cpu(), reference[name]))
    print("eager float32 vs float64, worst over N = 5, 16, 64:", worst)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["block", "all"])
@pytest.mark.parametrize("N,special", CASES)
def test_backward_matches_eager_autograd_and_float64(dev, eager_float64_error, N, special, which):
    """Random cotangents on the packed block alone (the benchmark's case) and on all four tensors plus the block: the raw gradients against
    eager float32 autograd on the device, and against float64 autograd on the CPU to three times the error the eager float32 path keeps:
    on the same inputs and cotangents, or over the file's inputs (eager_float64_error), whichever is larger."""
    native, eager, reference = three_ways(dev, N, special, which)
    tag = f"test_backward_matches_eager_autograd_and_float64[{N}-{special}-{which}]"
    errors = {}
    for name in NAMES:
        bound = BACKWARD_BOUND[which][name]
        error = margin(tag, name + " vs eager", relative(native[name], eager[name]), bound if bound > 0 else 1e-30)
        native_error, eager_error = relative(native[name].cpu(), reference[name]), relative(eager[name].cpu(), reference[name])
        print(f"{tag}: {name}: vs eager {error:.3e}; vs float64: native {native_error:.3e}, eager {eager_error:.3e}")
        errors[name] = (error, native_error, eager_error)
        assert torch.isfinite(native[name]).all()
    assert all(errors[name][0] <= BACKWARD_BOUND[which][name] for name in NAMES), errors
    assert all(errors[name][1] <= 3.0 * max(errors[name][2], eager_float64_error[which][name]) for name in NAMES), (errors, eager_float64_error[which])


@pytest.mark.gpu
def test_the_block_feeds_the_hot_step_kernel(dev):
    """A box-only silhouette_step of 64 rays at the full shape (N = 16, S = 64) with VSRD_FLAG_YAW_GRADIENTS, which runs the hot kernel only
    over fields whose rotations pass field_bounds' test for exact rotations about y: the native block and the eager cat give the same loss
    and raw gradients bit for bit (the blocks being equal), and the entries the flag drops stay exact zeros."""
    from vsrd_amd import fields, rendering
    N, S, R = 16, 64, 64
    g = torch.Generator().manual_seed(5)
    raws = (torch.randn(1, N, 3, generator=g) * 0.5, torch.randn(1, N, 3, generator=g) * 0.5, torch.randn(1, N, 2, generator=g))
    raws[0][..., 2] = torch.empty(N).uniform_(-2.0, -0.5, generator=g)             # 12 to 38 m deep
    m = module(dev, [t[0] for t in raws])
    with torch.no_grad():
        centres = m()["locations"][0].cpu()
    aim = centres[torch.randint(0, N, (R,), generator=g)] + torch.randn(R, 3, generator=g) * 0.7
    directions = torch.nn.functional.normalize(aim, dim=-1).to(dev)
    origins, targets = torch.zeros(R, 3, device=dev), torch.rand(R, N, generator=g).to(dev)
    u = torch.rand(R, S, generator=g).to(dev), torch.rand(R, S, generator=g).to(dev)
    results = []
    for forward in (native_forward, eager_forward):
        out = forward(m)
        block = fields.FieldBlock(out["block"], 0.4, None, None, yaw_gradients=True)
        loss = rendering.silhouette_step(block, origins, directions, targets, (0.0, 100.0), S, 0.4, 0.4, u_coarse=u[0], u_fine=u[1])
        block_gradient = torch.autograd.grad(loss, out["block"], retain_graph=True)[0]
        results.append((loss.detach().clone(), block_gradient, raw_gradients(m, dict(loss=loss), dict(loss=torch.ones_like(loss)))))
    (native_loss, native_block, native), (eager_loss, eager_block, eager) = results
    assert float(native_block.abs().max()) > 0 and float(native_block[:, [4, 6, 7, 8, 10]].abs().max()) == 0.0
    assert torch.equal(native_loss, eager_loss) and torch.equal(native_block, eager_block)
    for name in NAMES:
        bound = BACKWARD_BOUND["block"][name]
        assert relative(native[name], eager[name]) <= bound


@pytest.mark.gpu
def test_module_behaviour(dev, monkeypatch):
    """The dict keeps its keys, shapes, dtypes and contiguity; state_dict round-trips; two forward / backward calls accumulate into .grad
    as torch does; the CPU module and a float64 module run without the library."""
    from vsrd_amd import _lib, models
    raws = raw_parameters(5, None)
    m = module(dev, raws)
    out, eager = m(), eager_forward(m)
    assert list(out) == ["boxes_3d", "locations", "dimensions", "orientations", "embeddings"] and out["embeddings"] is m.embeddings
    for key in ("boxes_3d", "locations", "dimensions", "orientations"):
        assert out[key].shape == eager[key].shape and out[key].dtype == torch.float32 and out[key].is_contiguous() and out[key].requires_grad
    assert sorted(m.state_dict()) == ["dimension_range", "dimensions", "embeddings", "location_range", "locations", "orientations"]
    copy = models.BoxParameters3D(1, 5).to(dev)
    copy.load_state_dict(m.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(copy().values(), out.values()))
    # gradient accumulation over two calls
    grads = cotangents(native_forward(m), "all", 3)
    once = raw_gradients(m, native_forward(m), grads)
    for p in (m.locations, m.dimensions, m.orientations):
        p.grad = None
    for _ in range(2):
        o = native_forward(m)
        torch.autograd.backward([o[k] for k in grads], [grads[k] for k in grads])
    for name in NAMES:
        assert torch.equal(getattr(m, name).grad, once[name] + once[name])
    with torch.no_grad():
        assert not m()["locations"].requires_grad
    # modules the native path does not apply to never reach the library
    def refuse(*args, **kwargs):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)
    for other in (module("cpu", raws), module(dev, raws, torch.float64)):
        result = other()
        assert result["locations"].dtype == other.locations.dtype and result["boxes_3d"].shape == (1, 5, 8, 3)
        result["boxes_3d"].sum().backward()
        assert other.locations.grad is not None
    batch = models.BoxParameters3D(2, 5).to(dev)
    assert batch()["orientations"].shape == (2, 5, 3, 3)
    with pytest.raises(AssertionError, match="the library was loaded"):
        m()


def test_refusals():
    """N = 0, N above VSRD_MAX_INSTANCES and null pointers: VSRD_E_INVALID_ARGUMENT before any launch (made-up addresses are never followed).
    The backward's cotangents may be null, each of them."""
    import __graft_entry__
    __graft_entry__.build()
    from vsrd_amd import _lib
    lib = _lib.load()
    assert lib.vsrd_abi_version() == 12                          # added within ABI 12: probe for the symbols
    invalid = _lib.E_INVALID_ARGUMENT
    for N in (0, -1, _lib.MAX_INSTANCES + 1, 1 << 20):
        assert lib.vsrd_box_decode_forward(*([DUMMY] * 5), N, *([DUMMY] * 5), None) == invalid
        assert lib.vsrd_box_decode_backward(*([DUMMY] * 5), N, *([DUMMY] * 5), *([DUMMY] * 3), None) == invalid
    for missing in range(10):
        pointers = [None if k == missing else DUMMY for k in range(10)]
        assert lib.vsrd_box_decode_forward(*pointers[:5], 3, *pointers[5:], None) == invalid
    for missing in list(range(5)) + [10, 11, 12]:
        pointers = [None if k == missing else DUMMY for k in range(13)]
        assert lib.vsrd_box_decode_backward(*pointers[:5], 3, *pointers[5:], None) == invalid
