"""The C ABI of the patch-correlation loss (include/vsrd_hip.h: vsrd_grayscale_images, vsrd_patch_correlation_workspace_bytes, _forward,
_backward), met without a device: the symbols and their prototypes, the workspace query, and every refusal that happens before a launch --
checked with null pointers and made-up addresses, which a call that refuses never follows."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vsrd_grayscale_images", "vsrd_patch_correlation_workspace_bytes", "vsrd_patch_correlation_forward", "vsrd_patch_correlation_backward")
DUMMY = 4096                     # a made-up non-null address: a refused call reads nothing behind it


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from vsrd_amd import _lib
    return _lib.load()


def _config(**changes):
    from vsrd_amd import _lib
    values = dict(num_views=17, num_rays=100, height=94, width=352, patch_width=11, patch_height=11, top_k=4, target_view=0,
                  sample_epsilon=1e-6, correlation_epsilon=1e-12)
    values.update(changes)
    return _lib.PatchCorrelationConfig(**values)


def _forward(lib, config, workspace_bytes=1 << 20, **null):
    p = lambda name: None if name in null else DUMMY
    return lib.vsrd_patch_correlation_forward(config, p("gray"), p("intrinsics"), p("extrinsics"), p("pixels"), p("positions"), p("normals"),
                                              p("converged"), p("workspace"), workspace_bytes, p("loss"), p("stats"), None, None, None, None)


def _backward(lib, config, workspace_bytes=1 << 20, **null):
    p = lambda name: None if name in null else DUMMY
    return lib.vsrd_patch_correlation_backward(config, p("gray"), p("intrinsics"), p("extrinsics"), p("pixels"), p("positions"), p("normals"),
                                               p("converged"), p("workspace"), workspace_bytes, p("stats"), p("grad_loss"), p("grad_positions"),
                                               p("grad_normals"), None)


def test_symbols_and_prototypes(lib):
    from vsrd_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    void, size, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32
    config = ctypes.POINTER(_lib.PatchCorrelationConfig)
    assert _lib.SIGNATURES["vsrd_grayscale_images"] == (i32, [void, i32, i32, i32, void, void])
    assert _lib.SIGNATURES["vsrd_patch_correlation_workspace_bytes"] == (size, [i32, i32, i32])
    assert _lib.SIGNATURES["vsrd_patch_correlation_forward"] == (i32, [config] + [void] * 8 + [size] + [void] * 6)
    assert _lib.SIGNATURES["vsrd_patch_correlation_backward"] == (i32, [config] + [void] * 8 + [size] + [void] * 5)
    assert lib.vsrd_abi_version() == 12                          # added within ABI 12: probe for the symbols


def test_config_matches_the_header():
    from vsrd_amd import _lib
    header = open(os.path.join(ROOT, "include", "vsrd_hip.h")).read()
    body = re.search(r"typedef struct vsrd_patch_correlation_config \{(.*?)\} vsrd_patch_correlation_config;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for kind, names in re.findall(r"(int32_t|float)\s+([\w\s,]+);", body):
        declared += [(name.strip(), kind) for name in names.split(",")]
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(name, ctype[kind]) for name, kind in declared] == list(_lib.PatchCorrelationConfig._fields_)
    defines = dict(re.findall(r"^#define VSRD_PATCH_MAX_(\w+) (\d+)", header, flags=re.M))
    assert (int(defines["VIEWS"]), int(defines["PIXELS"]), int(defines["RAYS"])) == (_lib.PATCH_VIEWS, _lib.PATCH_PIXELS, _lib.PATCH_RAYS) == (32, 256, 65535)


def test_workspace_query(lib):
    query = lib.vsrd_patch_correlation_workspace_bytes
    base = query(17, 100, 121)
    assert base > 0
    assert query(18, 100, 121) > base and query(32, 100, 121) > query(18, 100, 121)           # grows with V
    assert query(17, 101, 121) > base and query(17, 65535, 121) > query(17, 101, 121)         # ... with R
    # ... and never shrinks with P: the patches live in LDS, so P is validated with the shape and adds no bytes today
    assert query(17, 100, 256) >= base >= query(17, 100, 1) > 0
    for V, R, P in [(0, 100, 121), (33, 100, 121), (17, 0, 121), (17, 65536, 121), (17, 100, 0), (17, 100, 257), (-1, -1, -1)]:
        assert query(V, R, P) == 0


@pytest.mark.parametrize("changes", [
    dict(top_k=0), dict(top_k=18), dict(num_views=0), dict(num_views=33, top_k=4), dict(num_views=3, top_k=4),
    dict(patch_width=0), dict(patch_height=0), dict(patch_width=16, patch_height=17), dict(patch_width=257, patch_height=1),
    dict(patch_width=-1, patch_height=-1), dict(num_rays=0), dict(num_rays=65536), dict(target_view=-1), dict(target_view=17),
    dict(height=1), dict(width=1), dict(height=0), dict(width=-5),
], ids=lambda changes: ",".join(f"{key}={value}" for key, value in changes.items()))
def test_limits_are_refused_before_a_launch(lib, changes):
    from vsrd_amd import _lib
    config = _config(**changes)
    assert _forward(lib, config) == _lib.E_INVALID_ARGUMENT
    assert _backward(lib, config) == _lib.E_INVALID_ARGUMENT


def test_limits_themselves_pass_the_shape_check(lib):
    """At the limits the shape is accepted: the call gets as far as the workspace check."""
    from vsrd_amd import _lib
    for changes in [dict(num_views=32, top_k=32), dict(patch_width=16, patch_height=16), dict(patch_width=256, patch_height=1), dict(num_rays=65535),
                    dict(num_views=1, top_k=1), dict(patch_width=1, patch_height=1), dict(num_rays=1), dict(height=2, width=2)]:
        assert _forward(lib, _config(**changes), workspace_bytes=1) == _lib.E_WORKSPACE
        assert _backward(lib, _config(**changes), workspace_bytes=1) == _lib.E_WORKSPACE


def test_null_pointers_and_short_workspace(lib):
    from vsrd_amd import _lib
    config = _config()
    need = lib.vsrd_patch_correlation_workspace_bytes(17, 100, 121)
    assert lib.vsrd_patch_correlation_forward(None, *([DUMMY] * 8), 1 << 20, DUMMY, DUMMY, None, None, None, None) == _lib.E_INVALID_ARGUMENT
    assert lib.vsrd_patch_correlation_backward(None, *([DUMMY] * 8), 1 << 20, *([DUMMY] * 4), None) == _lib.E_INVALID_ARGUMENT
    for name in ("gray", "intrinsics", "extrinsics", "pixels", "positions", "normals", "converged"):
        assert _forward(lib, config, **{name: True}) == _lib.E_INVALID_ARGUMENT
        assert _backward(lib, config, **{name: True}) == _lib.E_INVALID_ARGUMENT
    assert _forward(lib, config, workspace_bytes=need - 1) == _lib.E_WORKSPACE
    assert _backward(lib, config, workspace_bytes=need - 1) == _lib.E_WORKSPACE
    assert _forward(lib, config, workspace_bytes=0) == _lib.E_WORKSPACE
    assert _forward(lib, config, workspace=True) == _lib.E_WORKSPACE
    for name in ("loss", "stats"):                               # with a workspace of the right size: the outputs, still before a launch
        assert _forward(lib, config, workspace_bytes=need, **{name: True}) == _lib.E_INVALID_ARGUMENT
    for name in ("stats", "grad_loss", "grad_positions", "grad_normals"):
        assert _backward(lib, config, workspace_bytes=need, **{name: True}) == _lib.E_INVALID_ARGUMENT


def test_grayscale_arguments(lib):
    from vsrd_amd import _lib
    assert lib.vsrd_grayscale_images(None, 2, 24, 40, DUMMY, None) == _lib.E_INVALID_ARGUMENT
    assert lib.vsrd_grayscale_images(DUMMY, 2, 24, 40, None, None) == _lib.E_INVALID_ARGUMENT
    for V, H, W in [(0, 24, 40), (2, 0, 40), (2, 24, 0), (65536, 24, 40)]:
        assert lib.vsrd_grayscale_images(DUMMY, V, H, W, DUMMY, None) == _lib.E_INVALID_ARGUMENT
