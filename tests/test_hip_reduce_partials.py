"""The deterministic second stage of the adjoint launches (csrc/render_kernels.h: reduce_partials_kernel, and in front of it
reduce_partials_residues_kernel wherever the workspace has room for the residues) as an exact check on the device's own numbers: run a
step, read the per-wave partial table back from the workspace, re-sum it on the host in float32 in the documented order -- thread t of
256 adds rows t, t + 256, ... in ascending order starting from +0, wave_sum's tree over each wave's 64 sums (wave.h: pairs, quads, half
rows, rows, two rows, four), then the four wave totals in order (+ `extra`) -- and compare bit for bit with what the launch returned.
Needs a real MI355X: ``-m gpu``.

A launch's table has one row per wave of its grid, and the grids are whole workgroups of four waves (api.hip: plan): the row counts
around the 256 residues are 252, 256 and 260, the smallest is 4.  The one-ray-per-wave launches of 1, 3, 255 and 257 rays leave that many
live rows in tables of 4, 4, 256 and 260."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345            # a quiet NaN no kernel writes: a table read with the wrong row count does not sum to the launch's result


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def resum(table, extra=None):
    """[rows, columns] float32 -> [columns]: reduce_partials_kernel's additions in its order."""
    table = np.ascontiguousarray(table, dtype=np.float32)
    rows, columns = table.shape
    acc = np.zeros((256, columns), np.float32)
    for first in range(0, rows, 256):
        chunk = table[first:first + 256]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    level = acc.reshape(4, 64, columns)
    while level.shape[1] > 1:
        level = level[:, 0::2] + level[:, 1::2]
    total = np.zeros(columns, np.float32)
    for wave in range(4):
        total = total + level[wave, 0]
    total = total + (np.zeros(columns, np.float32) if extra is None else np.asarray(extra, np.float32))
    assert total.dtype == np.float32
    return torch.from_numpy(total)


def scene(seed, N, R, S):
    g = torch.Generator().manual_seed(seed)
    loc = torch.stack([torch.empty(N).uniform_(-6, 6, generator=g), torch.empty(N).uniform_(-1.0, 1.5, generator=g),
                       torch.empty(N).uniform_(8, 30, generator=g)], -1)
    dim = torch.stack([torch.empty(N).uniform_(0.75, 1.0, generator=g), torch.empty(N).uniform_(0.75, 1.0, generator=g),
                       torch.empty(N).uniform_(1.5, 2.5, generator=g)], -1)
    yaw = torch.empty(N).uniform_(-3.1, 3.1, generator=g)
    rot = torch.stack([torch.stack([torch.cos(yaw), torch.zeros(N), torch.sin(yaw)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                       torch.stack([-torch.sin(yaw), torch.zeros(N), torch.cos(yaw)], -1)], -2)
    target = loc[torch.randint(0, N, (R,), generator=g)] + torch.randn(R, 3, generator=g) * 0.7
    return dict(loc=loc, dim=dim, rot=rot, origins=torch.zeros(R, 3), directions=torch.nn.functional.normalize(target, dim=-1),
                targets=torch.rand(R, N, generator=g))


def marked_workspace(dev, N, residual=False, step_shape=None):
    """The launch's workspace tensor, every word set to the sentinel."""
    from vsrd_amd.rendering import renderers
    buffer = renderers.current_workspace().adjoint(dev, N, residual, step_shape)
    buffer.view(torch.int32).fill_(SENTINEL)
    return buffer


def words(buffer, first, count):
    return buffer.view(torch.float32)[first:first + count].cpu().numpy()


# (N, S, rays, one ray per wave, rows of the table)
BOX_STEPS = [(3, 16, 1, True, 4), (3, 16, 3, True, 4), (16, 16, 255, True, 256), (3, 16, 256, True, 256), (16, 16, 257, True, 260),
             (3, 16, 13, False, 4), (16, 16, 40, False, 12), (3, 16, 1005, False, 252), (16, 16, 1024, False, 256), (3, 16, 1030, False, 260),
             (16, 64, 4100, False, 1028), (3, 20, 5000, False, 1252)]


@pytest.mark.parametrize("N,S,R,wave_per_ray,rows", BOX_STEPS)
def test_box_step_sums_its_partial_table_in_the_documented_order(dev, N, S, R, wave_per_ray, rows):
    """A box-only silhouette_step: the gradient of the packed block and the loss (the second table of the same launch: one number per wave)
    are the host's re-sum of the table bit for bit.  1028 and 1252 rows: more than four rows per residue, a last pass over 4 and over 228
    of the 256 residues; N = 16: 256 columns, N = 3: 48."""
    from vsrd_amd import fields, rendering
    from vsrd_amd.rendering import renderers
    sc = scene(40 + R, N, R, S)
    row = 16 * N
    buffer = marked_workspace(dev, N)
    renderers.STEP_WAVE_PER_RAY = wave_per_ray
    try:
        inst = fields.pack_instances(sc["loc"], sc["rot"], sc["dim"]).to(dev).requires_grad_(True)
        block = fields.FieldBlock(inst, 0.4, None, None, yaw_gradients=True)
        loss = rendering.silhouette_step(block, sc["origins"].to(dev), sc["directions"].to(dev), sc["targets"].to(dev), (0.0, 100.0), S, 0.4, 0.4, seed=3)
        gradient = torch.autograd.grad(loss, inst)[0]
    finally:
        renderers.STEP_WAVE_PER_RAY = False
    table = words(buffer, 0, rows * row).reshape(rows, row)
    loss_table = words(buffer, rows * row, rows).reshape(rows, 1)
    assert np.isfinite(table).all() and np.isfinite(loss_table).all() and float(np.abs(table).max()) > 0
    assert torch.equal(gradient.cpu().reshape(-1), resum(table))
    assert torch.equal(loss.detach().cpu().reshape(1), resum(loss_table))


def test_two_launch_backward_sums_its_partial_table_in_the_documented_order(dev):
    """render_hierarchical + backward on a box-only field (vsrd_render_backward, the rows kernels): one table, no loss."""
    from vsrd_amd import fields, rendering
    N, S, R, rows = 16, 16, 2060, 516
    sc = scene(7, N, R, S)
    row = 16 * N
    inst = fields.pack_instances(sc["loc"], sc["rot"], sc["dim"]).to(dev).requires_grad_(True)
    labels = rendering.render_hierarchical(fields.FieldBlock(inst, 0.4, None, None), sc["origins"].to(dev), sc["directions"].to(dev), (0.0, 100.0), S, 0.4, 0.4,
                                           seed=3)["labels"]
    buffer = marked_workspace(dev, N)
    (labels * sc["targets"].to(dev)).sum().backward()
    table = words(buffer, 0, rows * row).reshape(rows, row)
    assert np.isfinite(table).all() and float(np.abs(table).max()) > 0
    assert torch.equal(inst.grad.cpu().reshape(-1), resum(table))


def test_residual_step_adds_extra_and_sums_two_loss_columns(dev):
    """A small residual step (N = 2, 64 rays, S = 16: one round, 16 workgroups of four waves): the box gradient is the re-sum of the 64
    rows plus `extra` (the MLP's position adjoints chained into t and R: api.hip, lay_out's box_extra), the two loss terms are the two
    columns of the second table."""
    from vsrd_amd import _lib, fields, rendering
    N, S, R, rows = 2, 16, 64, 64
    sc = scene(11, N, R, S)
    row = 16 * N
    g = torch.Generator().manual_seed(12)
    mlp = (torch.randn(N, _lib.MLP_WEIGHTS, generator=g) * 0.1).to(dev).requires_grad_(True)
    inst = fields.pack_instances(sc["loc"], sc["rot"], sc["dim"]).to(dev).requires_grad_(True)
    buffer = marked_workspace(dev, N, True, (S, R))
    loss, terms = rendering.silhouette_step(fields.FieldBlock(inst, 0.4, mlp, None), sc["origins"].to(dev), sc["directions"].to(dev), sc["targets"].to(dev),
                                            (0.0, 100.0), S, 0.4, 0.4, seed=3, eikonal_ratio=0.01, return_terms=True)
    gradient = torch.autograd.grad(loss, inst)[0]
    # lay_out: box partials [64][32] | loss partials [64][2] | jets 64 x (1 round x N x 64 + 1) float4 | box_extra [N][16]
    loss_at = rows * row
    extra_at = loss_at + 2 * rows + rows * (N * 64 + 1) * 4
    table, loss_table, extra = words(buffer, 0, rows * row).reshape(rows, row), words(buffer, loss_at, 2 * rows).reshape(rows, 2), words(buffer, extra_at, row)
    assert np.isfinite(table).all() and np.isfinite(loss_table).all() and np.isfinite(extra).all() and float(np.abs(extra).max()) > 0
    assert torch.equal(gradient.cpu().reshape(-1), resum(table, extra))
    assert torch.equal(terms.cpu().reshape(2), resum(loss_table))
