"""The host side of the photometric term of the frame loop (vsrd_amd/optimization.py; include/vsrd_hip.h: vsrd_frame_photometric): the
`FrameInputs.images` keyword, the configuration, every refusal that needs no device, and the C ABI's declarations."""
import dataclasses
import re

import pytest
import torch

from vsrd_amd import _lib, losses, optimization

V, H, W, N = 4, 24, 32, 2


def frame(images=True, hard_pixels=200):
    soft = torch.zeros(V, H, W, N)
    soft.view(V, H * W, N)[:, :hard_pixels, 0] = 0.9
    soft.view(V, H * W, N)[:, hard_pixels:hard_pixels + 50, 1] = 0.4          # soft, but in no hard mask
    return optimization.FrameInputs((H, W), torch.eye(3).repeat(V, 1, 1), torch.eye(4).repeat(V, 1, 1), soft, torch.zeros(V, N, 2, 2),
                                    torch.ones(V, N, dtype=torch.bool), images=torch.rand(V, 3, H, W) if images else None)


def config(**weights):
    return optimization.OptimizationConfig(num_rays=16, num_samples=8, loss_weights={**losses.LOSS_WEIGHTS, "photometric_loss": 0.5, **weights})


def test_images_are_an_init_only_keyword():
    names = [f.name for f in dataclasses.fields(optimization.FrameInputs)]
    assert names == ["image_size", "intrinsic_matrices", "extrinsic_matrices", "soft_masks", "boxes_2d", "visible_masks", "boxes_3d", "rectification_matrix"]
    inputs = frame()
    assert tuple(inputs.images.shape) == (V, 3, H, W)
    assert frame(images=False).images is None
    positional = optimization.FrameInputs(*[getattr(inputs, name) for name in names])          # the positional fields are what they were
    assert positional.images is None and positional.label_frame_ids is None


def test_config_defaults():
    cfg = optimization.OptimizationConfig()
    assert cfg.surface_num_rays == 100 and tuple(cfg.surface_patch_size) == (11, 11) and cfg.surface_top_k == 4
    assert cfg.loss_weights["photometric_loss"] == 0.0 and optimization.photometric_weight(cfg) == 0.0
    assert optimization.photometric_weight(config()) == 0.5


@pytest.mark.parametrize("what, inputs, cfg, match", [
    ("missing images", lambda: frame(images=False), lambda: config(), "images"),
    ("too few hard pixels", lambda: frame(hard_pixels=60), lambda: config(), "hard mask"),
    ("silhouette weight 0", lambda: frame(), lambda: config(silhouette_loss=0.0), "silhouette"),
    ("unknown loss key", lambda: frame(), lambda: config(photometric_los=1.0), "photometric_los"),
    ("too many rays", lambda: frame(), lambda: dataclasses.replace(config(), surface_num_rays=4096), "surface_num_rays"),
    ("top_k beyond the views", lambda: frame(), lambda: dataclasses.replace(config(), surface_top_k=V + 1), "top_k"),
    ("patch too large", lambda: frame(), lambda: dataclasses.replace(config(), surface_patch_size=(17, 17)), "surface_patch_size"),
    ("images of another shape", lambda: dataclasses.replace(frame(), images=torch.rand(V, 3, H, W + 1)), lambda: config(), "images of shape"),
])
@pytest.mark.parametrize("graph", [False, True])
def test_refusals_need_no_device(what, inputs, cfg, match, graph):
    with pytest.raises(ValueError, match=match):
        optimization.FrameOptimizer(inputs(), cfg(), "cuda:0", graph=graph)


def test_unknown_loss_key_is_refused_with_the_term_off():
    cfg = optimization.OptimizationConfig(loss_weights={**losses.LOSS_WEIGHTS, "photometric": 1.0})
    with pytest.raises(ValueError, match="unknown"):
        optimization.FrameOptimizer(frame(), cfg, "cuda:0")
    with pytest.raises(ValueError, match="unknown"):
        optimization.FrameBatch([frame()], cfg, "cuda:0")


def test_a_batch_refuses_the_term():
    with pytest.raises(ValueError, match="not batched"):
        optimization.FrameBatch([frame(), frame()], config(), "cuda:0")


def test_surface_rays_without_the_term():
    """(the check sits in front of anything that touches a device)"""
    loop = object.__new__(optimization.FrameOptimizer)
    loop._photometric, loop._graphs = None, {}
    with pytest.raises(ValueError, match="photometric term is off"):
        loop.step(surface_ray_indices=torch.zeros(4, dtype=torch.int64))


def test_header_declares_the_symbols_and_the_binding_reads_them():
    with open(_lib.HEADER_PATH) as file:
        text = file.read()
    assert "#define VSRD_ABI_VERSION 12" in text and _lib.ABI_VERSION == 12
    for name in ("vsrd_frame_photometric_workspace_bytes", "vsrd_frame_photometric", "vsrd_frame_photometric_finish"):
        assert re.search(rf"^(int32_t|size_t)\s+{name}\s*\(", text, flags=re.M), name
        assert name in _lib.SIGNATURES
    assert "typedef struct vsrd_frame_photometric_config" in text
    restype, arguments = _lib.SIGNATURES["vsrd_frame_photometric"]
    assert restype is _lib.ctypes.c_int32 and arguments[0] == _lib.ctypes.POINTER(_lib.FramePhotometricConfig)
    assert arguments[1] == _lib.ctypes.POINTER(_lib.PatchCorrelationConfig) and arguments[2] == _lib.ctypes.POINTER(_lib.Field)
    assert _lib.SIGNATURES["vsrd_frame_photometric_workspace_bytes"] == (_lib.ctypes.c_size_t, [_lib.ctypes.c_int32] * 5)
    limit = int(re.search(r"#define VSRD_PHOTOMETRIC_MAX_RAYS (\d+)", text).group(1))
    assert limit == _lib.PHOTOMETRIC_RAYS == 2048
    # the struct as the header lays it out: four 4-byte scalars, num_frames, padding, frame_stride
    assert _lib.ctypes.sizeof(_lib.FramePhotometricConfig) == 32 and _lib.FramePhotometricConfig.frame_stride.offset == 24
