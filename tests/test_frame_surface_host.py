"""The host side of vsrd_frame_surface: the binding against the header, the surface files and their PNG, the launcher's flags, and the row
declaration -- no GPU."""
import ctypes
import json
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vsrd_hip.h")
STRUCT = "vsrd_frame_surface_config"


def test_binding_has_the_prototype_and_the_struct():
    """The symbol and its structure are in the header and in _lib's table (which tests/test_host_logic.py::test_header_symbols_are_exported
    then holds against the library's exports); the ABI version has not moved."""
    from vsrd_amd import _lib
    header = open(HEADER).read()
    assert re.search(r"^int32_t\s+vsrd_frame_surface\s*\(", header, flags=re.M) and f"typedef struct {STRUCT}" in header
    assert re.search(r"^#define VSRD_ABI_VERSION 12$", header, flags=re.M) and _lib.ABI_VERSION == 12
    restype, argtypes = _lib.SIGNATURES["vsrd_frame_surface"]
    assert restype is ctypes.c_int32 and len(argtypes) == 17
    assert argtypes[:3] == [ctypes.POINTER(_lib.Field), ctypes.POINTER(_lib.RenderConfig), ctypes.POINTER(_lib.FrameSurfaceConfig)]
    assert argtypes[3:] == [ctypes.c_void_p] * 14
    assert _lib._HOST_STRUCTS[STRUCT] is _lib.FrameSurfaceConfig
    assert (_lib.FRAME_SURFACE_HARD_UNION, _lib.FRAME_SURFACE_SHADOWS) == tuple(int(re.search(r"#define VSRD_SURFACE_%s (\d+)u" % name, header).group(1))
                                                                   for name in ("HARD_UNION", "SHADOWS"))


def test_struct_matches_the_header(tmp_path):
    """The ctypes structure against the C compiler's view of the header: member names in declaration order, sizeof, and offsetof / sizeof of
    every member (the method of tests/test_host_logic.py::test_struct_matches_the_header)."""
    from vsrd_amd import _lib
    header = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (STRUCT, STRUCT), header, flags=re.S).group(1)
    declarations = [line for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if line.strip()]
    declared = [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", declarator).group(1) for line in declarations for declarator in line.split(",")]
    names = [name for name, _ in _lib.FrameSurfaceConfig._fields_]
    assert names == declared
    lines = [f'printf("{STRUCT} %zu 0\\n", sizeof({STRUCT}));']
    lines += [f'printf("{name} %zu %zu\\n", offsetof({STRUCT}, {name}), sizeof((({STRUCT}*)0)->{name}));' for name in declared]
    source = tmp_path / "layout.c"
    source.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vsrd_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(source), "-o", str(tmp_path / "layout")], check=True)
    rows = {key: (int(a), int(b)) for key, a, b in (line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                                                                            check=True).stdout.splitlines())}
    assert ctypes.sizeof(_lib.FrameSurfaceConfig) == rows[STRUCT][0]
    for name in names:
        member = getattr(_lib.FrameSurfaceConfig, name)
        assert (member.offset, member.size) == rows[name], name


def test_surface_config_defaults():
    """The shadow ray's default offset is twice the convergence criteria; the flags and the background's size follow the arguments."""
    from vsrd_amd import _lib, rendering
    config = rendering.surface_config(1, 3, 5, 20, 128, 0.01, 50.0)
    assert (config.view, config.num_views, config.height, config.width, config.num_iterations) == (1, 3, 5, 20, 128)
    assert config.shadow_offset == ctypes.c_float(2.0 * 0.01).value and config.convergence_criteria == ctypes.c_float(0.01).value
    assert config.flags == _lib.FRAME_SURFACE_HARD_UNION | _lib.FRAME_SURFACE_SHADOWS and config.background_pixels == 0 and config.alpha == 1.0
    config = rendering.surface_config(0, 1, 5, 20, 128, 0.01, None, shadow_offset=0.01, hard=False, shadows=False, background=True, alpha=0.5)
    assert config.flags == 0 and config.background_pixels == 100 and config.bounding_radius == 0.0 and config.shadow_offset == ctypes.c_float(0.01).value
    palette = rendering.surface_palette(14)
    assert palette.shape == (14, 3) and palette.dtype == torch.float32 and torch.equal(palette[12], palette[0]) and len(torch.unique(palette[:12], dim=0)) == 12
    assert len(rendering.SURFACE_LIGHT) == 3 and rendering.SURFACE_LIGHT[1] > 0 and rendering.SURFACE_LIGHT[2] > 0       # downwards and forwards: from above and behind


def _surface(rng, height=5, width=13):
    converged = rng.random((height, width)) < 0.5
    shadow = converged & (rng.random((height, width)) < 0.3)
    return converged, shadow, dict(converged_bits=torch.from_numpy(np.packbits(converged, axis=-1)), shadow_bits=torch.from_numpy(np.packbits(shadow, axis=-1)),
                                   instance=torch.from_numpy(np.where(converged, rng.integers(0, 4, (height, width)), 255).astype(np.uint8)),
                                   range=torch.from_numpy((rng.random((height, width)) * converged).astype(np.float32)),
                                   colors=torch.from_numpy(rng.integers(0, 256, (height, width, 3)).astype(np.uint8)),
                                   light=torch.tensor([0.3, 1.0, 0.6]), shape=(height, width), view=0)


def png_chunks(data):
    """[(type, payload)] of a PNG file's chunks, every CRC checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    chunks, at = [], 8
    while at < len(data):
        length, kind = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + length]
        assert struct.unpack(">I", data[at + 8 + length:at + 12 + length])[0] == zlib.crc32(kind + payload) & 0xFFFFFFFF
        chunks.append((kind, payload))
        at += 12 + length
    assert at == len(data)
    return chunks


def test_surface_files_round_trip_and_the_png_decodes(tmp_path):
    from vsrd_amd import formats, frames
    converged, shadow, surface = _surface(np.random.default_rng(0))
    paths = formats.save_frame_surface(str(tmp_path), surface)
    assert paths == (str(tmp_path / "surface" / "view_00.npz"), str(tmp_path / "surface" / "view_00.png"))
    assert sorted(os.listdir(tmp_path / "surface")) == ["view_00.npz", "view_00.png"]                               # (no temporary file left)
    for source in (paths[0], str(tmp_path)):
        loaded = formats.load_frame_surface(source)
        assert sorted(loaded) == ["converged_bits", "instance", "light", "range", "shadow_bits", "shape"] and loaded["shape"] == (5, 13)
        for key in ("converged_bits", "shadow_bits", "instance", "range", "light"):
            assert np.array_equal(loaded[key], surface[key].numpy()) and loaded[key].dtype == surface[key].numpy().dtype, key
        assert np.array_equal(frames.unpack_masks(loaded["converged_bits"][None], 13)[0], converged)
        assert np.array_equal(frames.unpack_masks(loaded["shadow_bits"][None], 13)[0], shadow)
    # the PNG: signature, IHDR (8-bit RGB, no interlace), IDAT rows of filter 0, IEND -- decoded with zlib alone
    chunks = png_chunks(open(paths[1], "rb").read())
    assert [kind for kind, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (13, 5, 8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(5, 1 + 13 * 3)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(5, 13, 3), surface["colors"].numpy())
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(paths[1]) as image:
            assert image.mode == "RGB" and image.size == (13, 5) and np.array_equal(np.asarray(image), surface["colors"].numpy())
    # another view gets files of its own; shapes that do not fit are refused before anything is written
    assert formats.save_frame_surface(str(tmp_path), surface, view=2)[1].endswith("view_02.png")
    for key, value in (("converged_bits", surface["converged_bits"][:, :1]), ("colors", surface["colors"][:4]), ("instance", surface["instance"][:, :5])):
        with pytest.raises(ValueError):
            formats.save_frame_surface(str(tmp_path / "bad"), dict(surface, **{key: value}))
    assert not os.path.exists(tmp_path / "bad" / "surface" / "view_00.npz")
    with pytest.raises(ValueError):
        formats.png_bytes(np.zeros((4, 4), dtype=np.uint8))


def test_row_declaration_and_planning():
    """surface() is the fifth _FrameOutput of the one table, on the path of the others: a batch's rows count its buffers only when the
    batch was built for them (its row switch), so rows without are as large as before."""
    from vsrd_amd import optimization
    V, N, H, W = 3, 5, 6, 20
    got = optimization._OUTPUTS["surface"].buffers(V, N, H, W)
    u8, f32 = torch.uint8, torch.float32
    assert [(key, tuple(shape), dtype, fill) for key, shape, dtype, fill in got] == [
        ("light", (3,), f32, 0.0), ("palette", (N, 3), f32, 0.0), ("background", (H * W, 3), u8, 0), ("converged_bits", (H, 3), u8, 0), ("shadow_bits", (H, 3), u8, 0),
        ("instance", (H * W,), u8, 255), ("range", (H * W,), f32, 0.0), ("colors", (H * W, 3), u8, 0)]
    assert optimization._OUTPUTS["surface"].last_step == "field block" and optimization._OUTPUTS["surface"].leading == "view_capacity"
    assert list(optimization._OUTPUTS) == ["labels", "masks", "metrics", "group_labels", "surface"]
    aligned = optimization.FrameArena.aligned
    extra = sum(aligned(optimization._buffer_bytes(shape, dtype)) for _, shape, dtype, _ in got)
    import inspect
    assert inspect.signature(optimization.FrameBatch._row_bytes).parameters["surface"].default is False
    assert inspect.signature(optimization.FrameBatch.__init__).parameters["surface"].default is False
    assert extra == sum(aligned(n) for n in (12, N * 12, H * W * 3, H * 3, H * 3, H * W, H * W * 4, H * W * 3))
    # the row switch: counted with surface=True and only then, whatever the other switches say
    config = optimization.OptimizationConfig()
    for label_views in (0, 2):
        for headed in (False, True):
            sizes = [optimization.FrameBatch._row_bytes((V, H, W, N), config, label_views, headed=headed, surface=surface) for surface in (False, True)]
            assert sizes[0] == optimization.FrameBatch._row_bytes((V, H, W, N), config, label_views, headed=headed) and sizes[1] - sizes[0] == extra


def _launcher(*arguments, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "vsrd_amd.launcher", *arguments], capture_output=True, text=True, cwd=ROOT, env=env, timeout=timeout)


def test_launcher_parses_the_flags_and_refuses_a_malformed_light(tmp_path):
    from vsrd_amd import launcher
    assert launcher.parse_light("") is None and launcher.parse_light("0.3,1,0.6") == (0.3, 1.0, 0.6) and launcher.parse_light("-1, 0 ,2e-1") == (-1.0, 0.0, 0.2)
    for bad in ("1,2", "1,2,3,4", "a,b,c", "0,0,0", "1,nan,0", "inf,0,0", ","):
        with pytest.raises(ValueError, match="--surface-light"):
            launcher.parse_light(bad)
    # refused before any rank starts: nothing is written, no rank's output appears
    for arguments, words in ((("--surface",), ("--surface", "--out")), (("--surface", "--out", str(tmp_path / "a"), "--selftest"), ("--selftest",)),
                             (("--surface", "--out", str(tmp_path / "b"), "--surface-light", "1,2"), ("--surface-light",)),
                             (("--surface", "--out", str(tmp_path / "c"), "--surface-light", "0,0,0"), ("--surface-light",)),
                             (("--out", str(tmp_path / "d"), "--surface-light", "1,2,3"), ("--surface-light", "--surface"))):
        done = _launcher("--gpus", "1", "--frames", "1", *arguments)
        assert done.returncode != 0 and all(word in done.stderr for word in words), (arguments, done.stderr[-500:])
        assert "Traceback" not in done.stderr and not done.stdout.strip()
    assert not any(os.path.exists(tmp_path / name) for name in "abcd")


def test_a_selftest_run_writes_nothing_unasked(tmp_path):
    """The launcher's CPU path with the new flags at their defaults: the line names no surface, and no frame folder holds one."""
    done = _launcher("--selftest", "--gpus", "1", "--frames", "3", "--selftest-seconds", "0.01", "--max-restarts", "0", "--out", str(tmp_path))
    assert done.returncode == 0, done.stderr[-3000:]
    line = [json.loads(l) for l in done.stdout.splitlines() if l.startswith("{")][-1]
    assert line["frames"] == 3 and "surface" not in line
    folders = [name for name in os.listdir(tmp_path) if name.startswith("frame_")]
    assert len(folders) == 3
    for name in folders:
        assert "surface" not in os.listdir(tmp_path / name) and not any(entry.endswith((".png", ".npz")) for entry in os.listdir(tmp_path / name))
