"""CPU-only checks of the host side: the C-ABI library loads and exports every declared symbol, the
ctypes structs match the header, the field recogniser flattens both our combinator objects and the
closure tree an unchanged scripts/main.py builds, and nothing in the product imports the oracle."""
import ctypes
import functools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from vsrd_amd import _lib
    return _lib.load()


def test_header_symbols_are_exported(lib):
    header = open(os.path.join(ROOT, "include", "vsrd_hip.h")).read()
    declared = set(re.findall(r"^(?:int32_t|size_t|const char\*)\s+(vsrd_\w+)\s*\(", header, flags=re.M))
    assert {"vsrd_render_forward", "vsrd_render_backward", "vsrd_render_hierarchical_forward", "vsrd_field_eval",
            "vsrd_ray_directions", "vsrd_sample_stratified", "vsrd_sample_importance"} <= declared
    from vsrd_amd import _lib
    assert declared == set(_lib.SIGNATURES), "ctypes binding and header disagree"
    for name in declared:
        assert getattr(lib, name) is not None
    # ... and the converse: the library exports no vsrd_* symbol the header does not declare (nm -D; the debug build's phase clocks aside)
    import subprocess
    exported = {line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", _lib.LIBRARY_PATH], capture_output=True, text=True, check=True).stdout.splitlines()
                if line.split()[-1].startswith("vsrd_") and " T " in line}
    assert exported - {"vsrd_debug_phase_cycles"} == declared, exported ^ declared
    assert lib.vsrd_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define VSRD_ABI_VERSION (\d+)", header).group(1))
    assert lib.vsrd_workspace_bytes(16, 0) == 16384 * 4 * 16 * 16 * 4
    # box partials + per-wave MLP partials (512 workgroups x 2 waves) + residual jets [wave][4 rounds][N][64] float4 + seeds [wave][8 rays][4][N][10][64]
    assert lib.vsrd_workspace_bytes(16, 1) == 16384 * 4 * 16 * 16 * 4 + 512 * 2 * 16 * 1617 * 4 + 512 * 2 * 4 * 16 * 64 * (16 + 8 * 28) + 512 * 2 * 16 * 16
    assert lib.vsrd_workspace_bytes(0, 0) == 0 and lib.vsrd_workspace_bytes(65, 0) == 0
    assert lib.vsrd_error_string(-1) == b"invalid argument"


def test_binding_is_read_from_the_header_and_refuses_what_it_does_not_know(monkeypatch, tmp_path):
    """_lib.SIGNATURES is parsed from the header's prototypes at import: the types of one prototype spelled out, a parameter type outside
    the binding's list is an error (no fall-back to a pointer or an int), and so is a missing header, by its path."""
    from vsrd_amd import _lib
    p = ctypes.c_void_p
    assert _lib.SIGNATURES["vsrd_sample_rays"] == (ctypes.c_int32, [p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, p, p, ctypes.c_size_t, p, p])
    assert _lib.SIGNATURES["vsrd_frame_epilogue"][1][5:9] == [ctypes.c_float] + [ctypes.POINTER(_lib.AdamTensors)] * 3
    assert _lib.SIGNATURES["vsrd_error_string"] == (ctypes.c_char_p, [ctypes.c_int32]) and _lib.SIGNATURES["vsrd_abi_version"] == (ctypes.c_int32, [])
    assert _lib.SIGNATURES["vsrd_ray_table_bytes"] == (ctypes.c_size_t, [ctypes.c_int64]) and _lib.SIGNATURES == _lib._signatures()
    for unknown in ("double x", "float** rows", "vsrd_field* field", "const vsrd_other* other", "const int32_t count", "int16_t n", "float"):
        with pytest.raises(_lib.VsrdHipError, match="no ctypes type"):
            _lib._argtype(unknown)
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "vsrd_hip.h"))
    with pytest.raises(_lib.VsrdHipError, match=re.escape(str(tmp_path / "include" / "vsrd_hip.h"))):
        _lib._signatures()


def test_workspace_sizes_are_the_parents(lib, monkeypatch):
    """The sizing contract of the C ABI, pinned.  Hosts size frame rows and arenas from these functions, so a change of the launch plans
    must not move a byte.  Every number below was recorded from the library of the commit BEFORE the launch planning was collapsed into
    plan_rows / lay_out (csrc/api.hip), not from the code under test.
    The sizing functions return the larger of the one-kernel floor (vsrd_workspace_bytes) and the split form's plan, so a plan's branch
    shows here only where its total exceeds the floor (some 41 000 ray-rounds per launch).  Above the floor: one, two and four rounds and
    the refused eight (S = 16 .. 129; distances 32 .. 258), a launch cut into chunks (N = 16, S = 64, R = 200000 against the 6 GiB seed
    budget), and each clamp of the item size: 4 (N = 1, one round, R = 60000: 60000 / 16384 = 3 -> 4, in both plans), 32 (N = 16,
    R = 30000: 58 -> 32) and 64 (N = 16, R = 100000: 195 -> 64).  NOT visible through these functions, and pinned only as the floor: the
    pair kernel on and off at two rounds (R = 2048 / 2049: 7 MB of seeds per instance against a floor of 74 MB), and the front kernels' LDS
    refusal at N = 64, S = 128 (the one-wave-per-ray plan is refused, the pair plan is taken and has the size the refused one would have).
    R = 0, N = 1 at one ray and the invalid arguments (0) complete the table.
    The patch correlation's and the photometric term's workspaces -- smallest and largest valid shapes, residual on and off, ray counts that
    are and are not multiples of four, and a count outside each limit (0) -- were recorded from the library of the commit BEFORE their
    sizes came out of the functions that carve them (patch_workspace, one_kernel_workspace in csrc/api.hip), likewise not from the code under test."""
    forced = [name for name in ("VSRD_PAIR_MAX_RAYS", "VSRD_SLOTS_PER_ITEM") if os.environ.get(name) is not None]
    for name in forced:
        monkeypatch.delenv(name)
    if forced:
        pytest.skip(f"{forced} set: the library froze its switches at the first call, the plans below are the defaults'")
    expected = {
        "vsrd_workspace_bytes": [
            ((1, 0), 4194304),
            ((1, 1), 73748480),
            ((16, 0), 67108864),
            ((16, 1), 1179975680),
            ((64, 1), 4719902720),
            ((0, 0), 0),
            ((65, 1), 0),
        ],
        "vsrd_residual_step_workspace_bytes": [
            ((1, 16, 60000), 208973008),
            ((16, 16, 60000), 1958398784),
            ((16, 32, 60000), 1958398784),
            ((16, 33, 30000), 1992084288),
            ((16, 64, 30000), 1992084288),
            ((16, 65, 15000), 2059455296),
            ((16, 100, 15000), 2059455296),
            ((16, 128, 15000), 2059455296),
            ((16, 129, 60000), 1179975680),
            ((16, 64, 2048), 1179975680),
            ((16, 64, 2049), 1179975680),
            ((16, 64, 200000), 6889404128),
            ((1, 16, 1), 73748480),
            ((16, 64, 100000), 6140264288),
            ((64, 128, 15000), 7377815184),
            ((64, 128, 1000), 4719902720),
            ((64, 100, 15000), 7377815184),
            ((3, 100, 132352), 3201244976),
            ((16, 64, 0), 1179975680),
            ((1, 100, 132352), 1067092592),
            ((0, 64, 100), 0),
            ((65, 64, 100), 0),
            ((16, 1, 100), 0),
            ((16, 257, 100), 0),
            ((16, 64, -1), 0),
        ],
        "vsrd_render_backward_workspace_bytes": [
            ((16, 0, 128, 60000), 67108864),
            ((1, 1, 32, 60000), 208947040),
            ((16, 1, 32, 60000), 1958228816),
            ((16, 1, 65, 60000), 1958228816),
            ((16, 1, 66, 30000), 1991914320),
            ((16, 1, 200, 20000), 2698975328),
            ((16, 1, 257, 20000), 2698975328),
            ((16, 1, 258, 20000), 1179975680),
            ((64, 1, 256, 20000), 7747658272),
            ((16, 1, 128, 200000), 7259602528),
            ((16, 1, 128, 0), 1179975680),
            ((1, 1, 2, 1), 73748480),
            ((0, 1, 128, 10), 0),
            ((16, 1, 1, 10), 0),
            ((16, 1, 513, 10), 0),
            ((16, 1, 128, -1), 0),
        ],
        "vsrd_hypernetwork_workspace_bytes": [
            ((1,), 235904),
            ((8,), 1812864),
            ((64,), 14428544),
            ((0,), 0),
            ((65,), 0),
        ],
        "vsrd_frame_scratch_bytes": [
            ((1, 1), 144),
            ((4, 8), 4608),
            ((32, 64), 294912),
            ((0, 1), 0),
            ((33, 1), 0),
            ((1, 65), 0),
        ],
        "vsrd_patch_correlation_workspace_bytes": [          # (views, rays, patch pixels)
            ((1, 1, 1), 104),
            ((32, 65535, 256), 525864),
            ((4, 512, 49), 4336),
            ((3, 1000, 35), 8192),
            ((0, 10, 9), 0),
            ((33, 10, 9), 0),
            ((2, 0, 9), 0),
            ((2, 65536, 9), 0),
            ((2, 10, 257), 0),
        ],
        "vsrd_frame_photometric_workspace_bytes": [          # (instances, residual, views, rays, patch pixels)
            ((1, 0, 1, 1, 1), 4195328),
            ((1, 1, 1, 1, 1), 73762304),
            ((64, 0, 32, 2048, 256), 268758784),
            ((64, 1, 32, 2048, 256), 4721053952),
            ((8, 1, 4, 512, 49), 590171136),
            ((8, 0, 4, 513, 49), 33634816),
            ((3, 1, 2, 1001, 35), 221438464),
            ((0, 0, 2, 10, 9), 0),
            ((65, 1, 2, 10, 9), 0),
            ((8, 1, 33, 10, 9), 0),
            ((8, 1, 2, 2049, 9), 0),
            ((8, 0, 2, 10, 257), 0),
        ],
    }
    for name, rows in expected.items():
        for args, size in rows:
            assert getattr(lib, name)(*args) == size, (name, args)


def test_constants_match_the_header():
    """The literal constants of the binding against the header's #defines, both ways round: every integer VSRD_<X> the binding has a name <X>
    for has that value, and every constant of the binding's families is defined in the header.  MAX_VIEWS, which the header does not
    define, against the frame glue's own limit: the ONE definition, in the header of the host checks, which the glue's header takes over."""
    from vsrd_amd import _lib
    header = open(os.path.join(ROOT, "include", "vsrd_hip.h")).read()
    defines = {name: int(value.rstrip("u"), 0) for name, value in re.findall(r"^#define VSRD_(\w+) \(?(-?(?:0x[0-9a-fA-F]+|\d+)u?)\)?(?:\s|$)", header, flags=re.M)}
    assert {"OK", "HYPER_WIDTH", "ABI_VERSION", "E_WORKSPACE", "FLAG_MLP_SPLIT_BF16", "MAX_LABEL_VIEWS"} <= set(defines)
    shared = [name for name in defines if hasattr(_lib, name)]
    for name in shared:
        assert getattr(_lib, name) == defines[name], name
    family = re.compile(r"(FLAG_|E_)\w+|MAX_INSTANCES|MAX_SAMPLES|MAX_LABEL_VIEWS|INSTANCE_STRIDE|MLP_WEIGHTS|HYPER_LAYERS|FRAME_HEADER_HAS_VIEWS|ABI_VERSION")
    named = [name for name in vars(_lib) if family.fullmatch(name)]
    assert sorted(named) == sorted(shared) and len(named) == 24
    checks, glue = (open(os.path.join(ROOT, "vsrd_amd", "csrc", name)).read() for name in ("host_checks.h", "frame_step.h"))
    assert _lib.MAX_VIEWS == int(re.search(r"constexpr int kFrameMaxViews = (\d+)", checks).group(1))
    assert "using vsrd_host::kFrameMaxViews;" in glue and "kFrameMaxViews =" not in glue


STRUCTS = {"Field": "vsrd_field", "RenderConfig": "vsrd_render_config", "FrameConfig": "vsrd_frame_config", "AdamTensors": "vsrd_adam_tensors",
           "Hypernetwork": "vsrd_hypernetwork", "FrameHeader": "vsrd_frame_header", "FrameMasksConfig": "vsrd_frame_masks_config"}


def _declared_members(struct):
    """The member names of `typedef struct <struct> {...}` in the header, in declaration order (`float height, width;` and
    `float location_lo[3], location_hi[3];` are two members each)."""
    header = open(os.path.join(ROOT, "include", "vsrd_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
    declarations = [line for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if line.strip()]
    return [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", declarator).group(1) for line in declarations for declarator in line.split(",")]


@pytest.fixture(scope="module")
def compiled_layout(tmp_path_factory):
    """The C compiler's view of include/vsrd_hip.h (gcc, one program for all structures): {"<struct>": sizeof, "<struct>.<member>":
    (offsetof, sizeof)} for every member the header declares."""
    import subprocess
    folder = tmp_path_factory.mktemp("layout")
    lines = []
    for struct in STRUCTS.values():
        lines.append(f'printf("{struct} %zu 0\\n", sizeof({struct}));')
        lines += [f'printf("{struct}.{name} %zu %zu\\n", offsetof({struct}, {name}), sizeof((({struct}*)0)->{name}));' for name in _declared_members(struct)]
    source = folder / "layout.c"
    source.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vsrd_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(source), "-o", str(folder / "layout")], check=True)
    rows = [line.split() for line in subprocess.run([str(folder / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()]
    return {key: (int(first), int(second)) for key, first, second in rows}


@pytest.mark.parametrize("binding", list(STRUCTS))
def test_struct_matches_the_header(compiled_layout, binding):
    """A ctypes structure against the C compiler's view of the header itself, not against numbers copied into the test: the member names in
    declaration order, sizeof the structure, and offsetof and sizeof of EVERY member."""
    from vsrd_amd import _lib
    structure, struct = getattr(_lib, binding), STRUCTS[binding]
    names = [name for name, _ in structure._fields_]
    assert names == _declared_members(struct)
    assert ctypes.sizeof(structure) == compiled_layout[struct][0]
    for name in names:
        member = getattr(structure, name)
        assert (member.offset, member.size) == compiled_layout[f"{struct}.{name}"], (struct, name)


def test_struct_layout_matches_header():
    """The sizes the ABI has had since its version 8, as literals (the members: test_struct_matches_the_header)."""
    from vsrd_amd import _lib
    assert ctypes.sizeof(_lib.RenderConfig) == 160 and ctypes.sizeof(_lib.FrameConfig) == 128 and ctypes.sizeof(_lib.Hypernetwork) == 24 + 24 * 40 + 16      # ABI 8


def _frame_refusals(_lib):
    """[(label, entry point, arguments, code)]: calls of the entry points that take a vsrd_frame_config, each refused before any HIP call.
    Pointers are dummies that are never dereferenced."""
    P = 0x1000
    full = dict(num_steps=3000, temperatures=(1.0, 0.1), std_deviations=(1.0, 0.1), loss_weights=(1.0, 1.0, 1.0), betas=(0.9, 0.999), adam_epsilon=1e-8, lr_gamma=0.999)

    def config(N=3, V=4, frames=None, **changes):
        return _lib.make_frame_config(N, V, (32.0, 64.0), 1.0e-6, [[-50.0, 1.0, 0.0], [50.0, 2.0, 100.0]], [[0.7, 0.7, 1.5], [1.0, 1.0, 2.5]], frames=frames,
                                      **dict(full, **changes))
    adam = _lib.AdamTensors(P, P, P, P, P)
    scratch = 4 * 3 * 36 * 4                   # vsrd_frame_scratch_bytes(4, 3)

    def prologue(c, first=P, out=P, scratch_pointer=P, scratch_bytes=scratch, tail=()):
        return [c, first, P, P, P, P, P, P, P, scratch_pointer, scratch_bytes, P, P, P, P, P, P, P, out, *tail, None]
    draw = (P, 4096, 64, 5, None, P)           # ray_table, count, num_rays, seed, remap, ray_indices
    entries = {          # name -> arguments(config, null first input, null required output)
        "vsrd_frame_prologue": lambda c, first=P, out=P: prologue(c, first, out),
        "vsrd_frame_prologue_with_header": lambda c, first=P, out=P: prologue(c, first, out, tail=(P,)),
        "vsrd_frame_prologue_sample": lambda c, first=P, out=P: prologue(c, first, out, tail=draw),
        "vsrd_frame_prologue_sample_with_header": lambda c, first=P, out=P: prologue(c, first, out, tail=(*draw, P)),
        "vsrd_frame_epilogue": lambda c, first=P, out=P: [c, first, P, P, P, 0.1, adam, adam, adam, P, P, P, out, P, None],
        "vsrd_frame_epilogue_with_header": lambda c, first=P, out=P: [c, first, P, P, P, 0.1, adam, adam, adam, P, P, P, out, P, P, None],
        "vsrd_frame_labels": lambda c, first=P, out=P: [c, first, P, P, P, P, P, P, P, P, out, P, P, P, None],
        "vsrd_frame_group_labels": lambda c, first=P, out=P, L=5: [c, first, P, P, L, P, P, P, P, P, P, P, out, P, P, P, None],
        "vsrd_frame_metrics": lambda c, first=P, out=P, gi=P: [c, first, P, P, P, P, P, gi, P, P, out, P, None],
    }
    steps = [name for name in entries if "prologue" in name or "epilogue" in name]
    cases = []
    for name, arguments in entries.items():
        for label, c in (("N = 0", config(N=0)), ("N = 65", config(N=65)), ("B = 2, stride 0", config(frames=(2, 0))), ("B = 2, stride 100", config(frames=(2, 100))),
                         ("B = 1025, stride 256", config(frames=(1025, 256)))):
            cases.append((label, name, arguments(c), -1))
        cases.append(("null first input", name, arguments(config(), first=None), -1))
        if name != "vsrd_frame_labels":            # (every output of vsrd_frame_labels may be null)
            cases.append(("null required output", name, arguments(config(), out=None), -1))
    for name in steps + ["vsrd_frame_labels"]:
        cases += [("V = 0", name, entries[name](config(V=0)), -1), ("V = 33", name, entries[name](config(V=33)), -1)]
    for name in steps:
        cases.append(("num_steps = 0", name, entries[name](config(num_steps=0)), -1))
    cases.append(("pd_indices without gt_indices", "vsrd_frame_metrics", entries["vsrd_frame_metrics"](config(), gi=None), -1))
    cases += [(f"L = {L}", "vsrd_frame_group_labels", entries["vsrd_frame_group_labels"](config(), L=L), -1) for L in (0, 4097)]
    for tail, name in (((), "vsrd_frame_prologue"), ((P,), "vsrd_frame_prologue_with_header")):
        cases.append(("scratch one byte short", name, prologue(config(), scratch_bytes=scratch - 1, tail=tail), -4))
        cases.append(("null scratch", name, prologue(config(), scratch_pointer=None, tail=tail), -4))
        cases.append(("null output and scratch one byte short", name, prologue(config(), out=None, scratch_bytes=scratch - 1, tail=tail), -1))
    # (the combined launches check the draw's arguments before the scratch: refused there, short of the LDS opt-in)
    for tail, name in (((P, 0, 64, 5, None, P), "vsrd_frame_prologue_sample"), ((P, 0, 64, 5, None, P, P), "vsrd_frame_prologue_sample_with_header")):
        cases.append(("count = 0 and scratch one byte short", name, prologue(config(), scratch_bytes=scratch - 1, tail=tail), -1))
    return cases


def test_frame_entry_points_refuse_what_the_parent_refused(lib):
    """What each entry point that takes a vsrd_frame_config refuses, and with which code -- the contract the single reader of that struct
    in csrc/api.hip (frame_shape / frame_args) must keep.  The rule of test_workspace_sizes_are_the_parents: every code below was recorded from
    a library built at the commit BEFORE that reader was introduced, not from the code under test.  The box count and the batch fields are
    refused by all nine entry points; the view count by the prologues, the epilogues and vsrd_frame_labels only; num_steps = 0 by the
    prologues and the epilogues only (vsrd_frame_metrics reads neither and is called with such configs); in the prologues an invalid
    argument is decided before the size of the scratch.  Every case returns before any HIP call (no GPU here); accepted calls are the GPU
    tests' (test_hip_frame_labels.py, test_hip_frame_group_labels.py, test_hip_frame_metrics.py: the configs those calls accept)."""
    from vsrd_amd import _lib
    cases = _frame_refusals(_lib)
    assert len(cases) == 93
    for label, name, arguments, code in cases:
        assert getattr(lib, name)(*arguments) == code, (name, label)
    assert lib.vsrd_frame_scratch_bytes(3, 4) == 1728 and lib.vsrd_frame_scratch_bytes(33, 4) == 0


def test_cpu_tensors_are_rejected_not_emulated(lib):
    from vsrd_amd import _lib
    with pytest.raises(_lib.VsrdHipError):
        _lib.ptr(torch.zeros(3))


def _main_py_style_field(loc, dim, rot, temperature, mlp=None, hyper=None):
    """Closures written like scripts/main.py:433-509 (nested ``wrapper`` functions), around OUR sdfs objects."""
    from vsrd_amd import rendering

    def residual_distance_field(distance_field):
        def wrapper(positions):
            return torch.sigmoid(distance_field(positions) - 1.0)     # never evaluated: the recogniser reads the closure
        return wrapper

    def residual_composition(distance_field, residual_distance_field):
        def wrapper(positions):
            return distance_field(positions) + residual_distance_field(positions)
        return wrapper

    def instance_field(distance_field, instance_label):
        def wrapper(positions):
            return distance_field(positions), instance_label
        return wrapper

    def soft_union(distance_fields, temperature):
        def wrapper(positions):
            return [f(positions) for f in distance_fields], temperature
        return wrapper

    members = []
    for i in range(loc.shape[0]):
        base = rendering.sdfs.box(dim[i])
        if mlp is not None:
            base = residual_composition(distance_field=base, residual_distance_field=residual_distance_field(
                distance_field=functools.partial(hyper, mlp[i])))
        members.append(rendering.sdfs.translation(rendering.sdfs.rotation(
            instance_field(distance_field=base, instance_label=dim.new_tensor(i, dtype=torch.long)), rot[i]), loc[i]))
    return soft_union(distance_fields=members, temperature=temperature)


def test_hypernetwork_pointer_block_follows_the_module_and_the_optimiser(lib):
    """optimization.hypernetwork_tensors: the vsrd_hypernetwork block points at the torch module's own parameters and at
    torch.optim.Adam's own state (created on the spot), group by group; other architectures are refused, and the entry points reject
    what they cannot run (no compute here: there is no GPU)."""
    from vsrd_amd import _lib, models, optimization
    net = models.HyperDistanceField(48, [16, 16, 16, 16], 256, [256, 256, 256, 256])
    embeddings = torch.nn.Parameter(torch.randn(1, 5, 256))
    lr = lambda v: torch.tensor(v)
    optimiser = torch.optim.Adam([dict(params=[embeddings], lr=lr(1e-3)), dict(params=list(net.parameters()), lr=lr(1e-4))], lr=lr(1e-3))
    block = optimization.hypernetwork_tensors(net, embeddings, optimiser, 0.99)
    assert (block.num_instances, block.num_outputs) == (5, _lib.MLP_WEIGHTS) and abs(block.lr_gamma - 0.99) < 1e-7
    assert (block.beta1, block.beta2) == (ctypes.c_float(0.9).value, ctypes.c_float(0.999).value)
    assert block.embeddings.parameter == embeddings.data_ptr() and block.embeddings.learning_rate == optimiser.param_groups[0]["lr"].data_ptr()
    linears = [b[0] for b in net.hypernetwork]
    for l, linear in enumerate(linears):
        state = optimiser.state[linear.weight_v]
        assert block.weight_v[l].parameter == linear.weight_v.data_ptr() and block.weight_g[l].parameter == linear.weight_g.data_ptr()
        assert block.weight_v[l].exp_avg == state["exp_avg"].data_ptr() and block.weight_v[l].step == state["step"].data_ptr()
        assert block.bias[l].learning_rate == optimiser.param_groups[1]["lr"].data_ptr()
    assert block.norm_weight[3].parameter == net.hypernetwork[3][1].weight.data_ptr()
    assert len(optimiser.state) == 1 + 5 * 3 + 4 * 2 and all(float(s["step"]) == 0.0 for s in optimiser.state.values())
    with pytest.raises(ValueError):                                   # not the reference's hypernetwork
        optimization.hypernetwork_tensors(models.HyperDistanceField(48, [16, 16, 16, 16], 256, [256, 256]), embeddings, optimiser, 0.99)
    assert lib.vsrd_hypernetwork_workspace_bytes(0) == 0 and lib.vsrd_hypernetwork_workspace_bytes(65) == 0
    assert lib.vsrd_hypernetwork_workspace_bytes(8) > 8 * 256 * 4 * 100
    assert lib.vsrd_hypernetwork_forward(block, None, 0, None, None, None) == -1           # VSRD_E_INVALID_ARGUMENT: no output buffer
    block.num_outputs = 100
    assert lib.vsrd_hypernetwork_backward_step(block, None, 0, None, 1.0, None) == -1


def test_recogniser_flattens_main_py_closures():
    from vsrd_amd import fields
    g = torch.Generator().manual_seed(0)
    loc = torch.randn(5, 3, generator=g).requires_grad_(True)
    dim = (torch.rand(5, 3, generator=g) + 0.5).requires_grad_(True)
    rot = torch.randn(5, 3, 3, generator=g).requires_grad_(True)
    block = fields.flatten(_main_py_style_field(loc, dim, rot, 0.37))
    assert block.instances.shape == (5, 16) and block.temperature == pytest.approx(0.37)
    assert block.mlp_weights is None and block.label_indices is None and not block.hard
    assert torch.equal(block.instances[:, 0:3], loc) and torch.equal(block.instances[:, 3:12], rot.reshape(5, 9))
    assert torch.equal(block.instances[:, 12:15], dim) and torch.all(block.instances[:, 15] == 0)
    # autograd reaches the original tensors through the packing
    gl, gd, gr = torch.autograd.grad(block.instances.sum(), [loc, dim, rot])
    assert torch.all(gl == 1) and torch.all(gd == 1) and torch.all(gr == 1)
    # residual variant: weights travel through functools.partial (main.py:541-544)
    mlp = torch.randn(5, 1617, generator=g)
    block = fields.flatten(_main_py_style_field(loc, dim, rot, 1.0, mlp=mlp, hyper=lambda w, x: x))
    assert torch.equal(block.mlp_weights, mlp)


def test_block_hand_over_is_scoped_to_one_wrapper_call():
    """fields.BlockHandOver (the module-level "last block" cache of round 3 could return a stale block): the block of
    main.py's pass 1 serves pass 2 only for the same closure object with every captured tensor at the same version; flatten()
    itself caches nothing, so a parameter update between steps -- through an optimiser, `.data` or a raw pointer -- is always seen."""
    from vsrd_amd import fields
    g = torch.Generator().manual_seed(1)
    loc = torch.randn(4, 3, generator=g).requires_grad_(True)
    dim = (torch.rand(4, 3, generator=g) + 0.5).requires_grad_(True)
    rot = torch.randn(4, 3, 3, generator=g).requires_grad_(True)
    field = _main_py_style_field(loc, dim, rot, 0.5)
    with torch.no_grad():
        block = fields.flatten(field)
    assert block.instances.requires_grad                          # built with autograd on even under no_grad: pass 2 differentiates it
    assert block.capture_key is not None                          # flatten's walk of the tree also serves the hand-over's comparison
    hand = fields.BlockHandOver(field, block)
    assert hand.key == block.capture_key and hand.take(field) is block
    assert hand.take(field) is None                               # single use: the block carries ONE autograd graph
    assert fields.BlockHandOver(field, block).take(_main_py_style_field(loc, dim, rot, 0.5)) is None      # another closure object (the next step's): no reuse
    hand = fields.BlockHandOver(field, block)
    with torch.no_grad():
        loc.add_(1.0)                                             # an in-place update bumps the version
    assert hand.take(field) is None
    # flatten() has no memory: the step after a `.data` update (no version bump) sees the new values
    loc.data.add_(5.0)
    assert torch.equal(fields.flatten(field).instances[:, 0:3], loc)
    fields.BLOCK_HAND_OVER = False
    try:
        assert fields.BlockHandOver(field, block).take(field) is None
    finally:
        fields.BLOCK_HAND_OVER = True


def test_recogniser_objects_labels_and_rejections():
    from vsrd_amd import fields, rendering
    loc, dim, rot = torch.zeros(3, 3), torch.ones(3, 3), torch.eye(3).repeat(3, 1, 1)
    members = [rendering.sdfs.translation(rendering.sdfs.rotation(fields.instance_field(rendering.sdfs.box(dim[i]), lab, 3), rot[i]), loc[i])
               for i, lab in enumerate([2, 0, 1])]
    block = fields.flatten(fields.soft_union(members, 0.5))
    assert block.label_indices.tolist() == [2, 0, 1]
    assert fields.flatten(fields.hard_union(members)).hard
    assert fields.flatten(rendering.sdfs.box(dim[0])).instances.shape == (1, 16)       # identity pose filled in
    with pytest.raises(fields.UnsupportedFieldError):
        fields.flatten(lambda p: p)
    with pytest.raises(fields.UnsupportedFieldError):                                   # rotation(translation(.)) is a different map
        fields.flatten(fields.soft_union([rendering.sdfs.rotation(rendering.sdfs.translation(rendering.sdfs.box(dim[0]), loc[0]), rot[0])], 1.0))
    with pytest.raises(fields.UnsupportedFieldError):
        fields.flatten(fields.soft_union([rendering.sdfs.box(dim[0])] * 65, 1.0))


def test_product_never_imports_the_oracle():
    for base, _, files in os.walk(os.path.join(ROOT, "vsrd_amd")):
        for name in files:
            if name.endswith((".py", ".h", ".hip")):
                text = open(os.path.join(base, name)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f"{name} imports the oracle"
                assert "/root/reference" not in text


def test_build_switches_are_the_ones_in_the_design_table():
    """Every VSRD_* name a preprocessor conditional of csrc/ tests has its line in DESIGN.md's "Build switches" table, and the table has
    no line for a switch that is gone."""
    tested = set()
    csrc = os.path.join(ROOT, "vsrd_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        for line in open(os.path.join(csrc, name)):
            directive = re.match(r"\s*#\s*(?:if|ifdef|ifndef|elif)\b([^/]*)", line)
            if directive:
                tested.update(re.findall(r"\bVSRD_\w+", directive.group(1)))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = re.search(r"^## [^\n]*Build switches\n(.*?)^## ", design, flags=re.M | re.S).group(1)
    listed = re.findall(r"^\| `(VSRD_\w+)` \|", section, flags=re.M)
    assert len(listed) == len(set(listed))
    assert tested and tested == set(listed)


def test_formats_match_reference_writers():
    """N4: KITTI label lines byte-for-byte against the reference's convert_predictions.save_prediction (golden g12), the
    prediction JSON layout, the checkpoint's detector state-dict layout and the multi-view confidence voting."""
    import json
    import tempfile
    import numpy as np
    from conftest import load_golden
    from vsrd_amd import formats, models
    g = load_golden("g12_formats")
    want = bytes(g["kitti_text"].numpy().astype(np.uint8)).decode()
    got = "".join(formats.kitti_label_line("car", b3, b2, s) for b3, b2, s in zip(g["boxes_3d"], g["boxes_2d"], g["scores"]))
    for a, b in zip(got.splitlines(), want.splitlines()):
        fa, fb = a.split(" "), b.split(" ")
        assert fa[0] == fb[0] and len(fa) == len(fb) == 16
        np.testing.assert_allclose([float(x) for x in fa[1:]], [float(x) for x in fb[1:]], rtol=1e-5, atol=1e-5)
    assert got.count("\n") == want.count("\n") == 3
    keys = bytes(g["state_keys"].numpy().astype(np.uint8)).decode().split("\n")
    mine = [f"{k}:{tuple(v.shape)}" for k, v in models.BoxParameters3D(1, 3).state_dict().items()]
    assert mine == keys                                           # loadable by make_predictions.py:61-66
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "predictions", "frame.json")
        formats.save_prediction(path, g["boxes_3d"], g["boxes_2d"], g["scores"])
        record = json.load(open(path))
        assert list(record) == ["boxes_3d", "boxes_2d", "confidences"] and list(record["boxes_3d"]) == ["car"]
        assert np.asarray(record["boxes_3d"]["car"]).shape == (3, 8, 3) and np.asarray(record["boxes_2d"]["car"]).shape == (3, 2, 2)
    # voting: prediction 0 overlaps target instance 1 in both views, prediction 1 overlaps instance 0 in one view
    pd = [torch.tensor([[[0., 0.], [10., 10.]], [[20., 20.], [30., 30.]]])] * 2
    gt = [torch.tensor([[[20., 20.], [30., 30.]], [[0., 0.], [10., 10.]]]), torch.tensor([[[0., 0.], [10., 5.]]])]
    conf, pd_idx, gt_idx = formats.multi_view_confidences(pd, gt, [torch.tensor([0, 1]), torch.tensor([1])])
    assert pd_idx.tolist() == [0, 1] and gt_idx.tolist() == [1, 0]
    np.testing.assert_allclose(conf.numpy(), [0.75, 1.0], rtol=1e-6)


def test_loss_library_matches_reference_g13():
    """a22: the vsrd.losses call surface (pure PyTorch) against the reference's own outputs."""
    from conftest import load_golden
    from vsrd_amd import loss_library as L
    g = load_golden("g13_loss_library")
    p, t = g["p"], g["t"]
    for name in ("cross_entropy", "binary_cross_entropy", "kl_divergence", "binary_kl_divergence", "js_divergence",
                 "binary_js_divergence", "focal_loss", "quality_focal_loss", "tversky_loss", "focal_tversky_loss"):
        torch.testing.assert_close(getattr(L, name)(p, t, reduction="none"), g["out_" + name], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(L.cross_entropy(p, t, dim=1), g["out_cross_entropy_dim1"], rtol=1e-5, atol=1e-6)
    a, b = g["img_a"], g["img_b"]
    torch.testing.assert_close(L.ssim_loss(a, b, reduction="none"), g["out_ssim_loss"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(L.photometric_loss(a, b, reduction="none"), g["out_photometric_loss"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(L.smoothness_loss(a[:, :1], b, reduction="none"), g["out_smoothness_loss"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(L.motion_smoothness_loss(a, reduction="none"), g["out_motion_smoothness_loss"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(L.motion_sparsity_loss(a - 0.5, reduction="sum"), g["out_motion_sparsity_loss"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(L.gaussian_nll(g["mean"], g["var"], g["target"], reduction="none"), g["out_gaussian_nll"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(L.student_nll(g["mean"], g["shape"], g["scale"], g["target"], reduction="none"), g["out_student_nll"], rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):
        L.cross_entropy(p, t, reduction="median")


def test_loss_library_rest_matches_reference_g18():
    """a22, second half: geometric_losses.py and the logit-space NLLs / Monte-Carlo energy scores of probabilistic_losses.py against
    the reference's outputs.  The energy scores sample from torch's global generator: seeding as the fixture generator did replays
    the reference's draws (one rsample([num_samples]) call per score)."""
    from conftest import load_golden
    from vsrd_amd import loss_library as L
    g = load_golden("g18_loss_library_rest")
    torch.testing.assert_close(L.rotation_consistency_loss(g["source"], g["target"], reduction="none"), g["out_rotation_consistency_loss"], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(L.translation_consistency_loss(g["source"], g["target"], reduction="none"), g["out_translation_consistency_loss"], rtol=1e-5, atol=1e-7)
    assert float(g["out_rotation_consistency_loss"][0]) < 1e-6 and float(g["out_translation_consistency_loss"][0]) < 1e-6      # target = source^-1
    torch.testing.assert_close(L.sampson_epipolar_distance(g["keypoints_1"], g["keypoints_2"], g["fundamental"][:, None], reduction="none"),
                               g["out_sampson_epipolar_distance"], rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(L.logit_gaussian_nll(g["mean"], g["var"], g["unit_targets"], reduction="none"), g["out_logit_gaussian_nll"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(L.logit_student_nll(g["mean"], g["shape"], g["scale"], g["unit_targets"], reduction="none"), g["out_logit_student_nll"], rtol=1e-4, atol=1e-5)
    n, seed = int(g["num_samples"]), int(g["seed"])
    for name, args in (("gaussian_energy_score", (g["mean"], g["var"], g["target_values"])),
                       ("student_energy_score", (g["mean"], g["shape"], g["scale"], g["target_values"])),
                       ("logit_gaussian_energy_score", (g["mean"], g["var"], g["unit_targets"])),
                       ("logit_student_energy_score", (g["mean"], g["shape"], g["scale"], g["unit_targets"]))):
        torch.manual_seed(seed)
        torch.testing.assert_close(getattr(L, name)(*args, num_samples=n, reduction="none"), g["out_" + name], rtol=1e-5, atol=1e-6)
    # reductions and the mean default, as the reference's @reduced decorator
    torch.manual_seed(seed)
    mean = L.gaussian_energy_score(g["mean"], g["var"], g["target_values"], num_samples=n)
    torch.testing.assert_close(mean, g["out_gaussian_energy_score"].mean(), rtol=1e-5, atol=1e-6)
    # every public name of the reference's vsrd/losses/*.py is there
    for name in ("cross_entropy binary_cross_entropy kl_divergence binary_kl_divergence js_divergence binary_js_divergence focal_loss quality_focal_loss "
                 "tversky_loss focal_tversky_loss rotation_consistency_loss translation_consistency_loss sampson_epipolar_distance ssim_loss photometric_loss "
                 "gaussian_nll student_nll gaussian_energy_score student_energy_score logit_gaussian_nll logit_student_nll logit_gaussian_energy_score "
                 "logit_student_energy_score smoothness_loss motion_smoothness_loss motion_sparsity_loss").split():
        assert callable(getattr(L, name)), name


def test_capture_gate_keeps_captures_alone():
    """optimization._CaptureGate: a capture runs alone; everything else a frame's thread calls into HIP (construction, eager steps, replay
    launches, graph destruction, host synchronisations) runs next to each other but never during a capture; a waiting capture goes before
    newcomers but does not stop a thread that is already inside from nesting; the garbage collector's non-blocking attempt is refused
    during a capture, inside the capturing thread too."""
    import threading
    import time
    from vsrd_amd import optimization
    gate = optimization._CaptureGate()
    log, inside = [], threading.Event()

    def other(tag, hold, nested=False):
        with gate.replaying():
            log.append(("in", tag))
            inside.set()
            time.sleep(hold)
            if nested:
                with gate:                                # nesting while a capture waits: must not deadlock
                    log.append(("nested", tag))
            log.append(("out", tag))

    first = threading.Thread(target=other, args=("a", 0.3, True))
    second = threading.Thread(target=other, args=("b", 0.0))
    first.start()
    assert inside.wait(5.0)
    second.start()                                        # next to "a": does not wait
    second.join(5.0)
    assert ("out", "b") in log and ("out", "a") not in log
    assert gate.acquire(blocking=False) is True           # ... and so may anybody else, the collector included
    gate.release()
    start = time.perf_counter()
    with gate.capture():                                  # waits for "a", which nests once on its way out
        assert ("nested", "a") in log and ("out", "a") in log and time.perf_counter() - start > 0.1
        assert gate.acquire(blocking=False) is False      # the collector inside the capturing thread: not now
        with gate:                                        # the capturing thread itself passes
            pass
        late = threading.Thread(target=other, args=("c", 0.0))
        late.start()
        time.sleep(0.1)
        assert ("in", "c") not in log                     # everybody else waits for the capture
        refused = []
        probe = threading.Thread(target=lambda: refused.append(gate.acquire(blocking=False)))
        probe.start(); probe.join(5.0)
        assert refused == [False]
    late.join(5.0)
    first.join(5.0)
    assert ("out", "c") in log and gate.capture_seconds > 0.0
    with gate:
        try:
            with gate.capture():                          # a capture inside a held section would wait for itself
                raise AssertionError("unreachable")
        except RuntimeError:
            pass


def test_steps_in_next_group_takes_whole_groups_inside_every_bound():
    """optimization._steps_in_next_group, the one rule by which FrameOptimizer.run and FrameBatch.run size their next graph launch: a whole
    group of ``steps_per_graph`` steps where the run, the phase and the log all leave room for one and the phase's one-step graph is held,
    a single step everywhere else."""
    import itertools
    from vsrd_amd.optimization import _steps_in_next_group
    grid = itertools.product(range(1, 15), [None, *range(1, 10)], [None, *range(1, 6)], (1, 2, 4), (False, True))
    for remaining, to_phase_end, to_log, steps_per_graph, held in grid:
        case = (remaining, to_phase_end, to_log, steps_per_graph, held)
        k = _steps_in_next_group(*case)
        bounds = [b for b in (remaining, to_phase_end, to_log) if b is not None]
        assert k in (1, steps_per_graph), case
        assert all(k <= b for b in bounds), case
        if not held:
            assert k == 1, case
        if held and all(steps_per_graph <= b for b in bounds):
            assert k == steps_per_graph, case
    # one walk by hand: 23 steps, the phase switch after 9, groups of 4, no log; a phase's one-step graph is held after its first four
    # single steps (three eager ones and the capture)
    warmup, position, singles, groups = 9, 0, {False: 0, True: 0}, []
    while position < 23:
        residual = position >= warmup
        k = _steps_in_next_group(23 - position, None if residual else warmup - position, None, 4, singles[residual] >= 4)
        singles[residual] += k == 1
        groups.append(k)
        position += k
    assert groups == [1, 1, 1, 1, 4, 1, 1, 1, 1, 1, 4, 4, 1, 1] and position == 23


def test_to_host_rebuilds_containers_and_leaves_the_rest():
    """formats.to_host: what launcher.main hands to torch.save for a frame optimised next to others -- every tensor a host copy, dicts /
    lists / tuples rebuilt with their types, everything else untouched."""
    import collections
    import torch
    from vsrd_amd import formats
    payload = collections.OrderedDict(step=7, models={"m": {"w": torch.arange(4.0).requires_grad_(True)}}, groups=[{"lr": 0.5, "params": (0, 1)}],
                                      metrics={}, name="frame")
    out = formats.to_host(payload)
    assert type(out) is collections.OrderedDict and list(out) == list(payload)
    assert out["step"] == 7 and out["name"] == "frame" and out["groups"] == [{"lr": 0.5, "params": (0, 1)}] and type(out["groups"][0]["params"]) is tuple
    w = out["models"]["m"]["w"]
    assert w.device.type == "cpu" and not w.requires_grad and torch.equal(w, torch.arange(4.0)) and w is not payload["models"]["m"]["w"]


def test_frame_arena_rows_share_one_layout():
    """optimization.FrameArena / FrameRow (frame batches, include/vsrd_hip.h ABI 8): every frame's copy of a buffer sits at the same offset of its
    row, rows are `stride` bytes apart, offsets are 256-byte aligned, views keep dtype and shape and alias the arena, and a row that runs out
    raises instead of walking into its neighbour."""
    from vsrd_amd import optimization
    arena = optimization.FrameArena(3, 10_000, "cpu")
    assert arena.stride % 256 == 0 and arena.stride >= 10_000 and arena.buffer.shape == (3, arena.stride)
    views = []
    for row in arena.rows:
        a = row.new((5, 3), torch.float32, fill=1.5)
        b = row.new(7, torch.int64, fill=2)
        c = row.new((), torch.float32, fill=0.25)
        d = row.adopt(torch.arange(6, dtype=torch.uint8).reshape(2, 3))
        views.append((a, b, c, d))
        assert a.shape == (5, 3) and a.dtype == torch.float32 and b.dtype == torch.int64 and c.shape == () and float(c) == 0.25
        assert torch.equal(d, torch.arange(6, dtype=torch.uint8).reshape(2, 3)) and all(t.is_contiguous() for t in (a, b, c, d))
    assert arena.rows[0].layout == arena.rows[1].layout == arena.rows[2].layout
    assert all(offset % 256 == 0 for offset, _ in arena.rows[0].layout)
    for k in range(4):           # frame f's buffer is exactly f * stride bytes behind frame 0's
        assert views[1][k].data_ptr() - views[0][k].data_ptr() == arena.stride and views[2][k].data_ptr() - views[0][k].data_ptr() == 2 * arena.stride
    views[1][0].fill_(9.0)       # rows do not overlap
    assert float(views[0][0].max()) == 1.5 and float(views[2][0].max()) == 1.5
    with pytest.raises(RuntimeError, match="exhausted"):
        arena.rows[0].new(10_000, torch.float32)


def test_frame_batch_item_slots_and_row_size(lib):
    """FrameBatch.item_slots: the MLP adjoint's work items grow with the batch (about 16384 items per launch); FrameBatch._row_bytes covers what a
    frame of the reference's size allocates (1.4 GB: directions, soft masks, the sampling table, and 0.8 GB of render workspace -- it is sized so that
    every form of the residual step fits, the one-kernel fallback's per-wave caches included)."""
    from vsrd_amd import optimization
    config = optimization.OptimizationConfig()
    assert [optimization.FrameBatch.item_slots(b, config, 8) for b in (1, 2, 4, 8, 16, 64)] == [4, 4, 8, 16, 32, 32]
    assert optimization.FrameBatch.item_slots(8, optimization.OptimizationConfig(num_samples=64), 16) == 16      # two rounds per ray, twice the instances
    row = optimization.FrameBatch._row_bytes((17, 376, 1408, 8), config)
    pixels = 17 * 376 * 1408
    assert row > pixels * (12 + 32 + 4) + lib.vsrd_ray_table_bytes(pixels) + lib.vsrd_residual_step_workspace_bytes(8, 100, 1000) and row < 3 << 29


def test_initial_draw_runs_on_one_thread_and_draws_the_same_values():
    """optimization._InitialDraw: the host-side draw of a frame's initial parameters runs on ONE intra-op thread (256 host cores made it 100 ms) and
    restores the count; the values do not depend on it."""
    from vsrd_amd import models, optimization
    before = torch.get_num_threads()

    def draw():
        torch.default_generator.manual_seed(7)
        return [p.detach().clone() for p in models.HyperDistanceField(48, [16, 16, 16, 16], 256, [256, 256, 256, 256]).parameters()]

    with optimization._initial_draw:
        assert torch.get_num_threads() == 1
        single = draw()
    assert torch.get_num_threads() == before
    for a, b in zip(single, draw()):
        assert torch.equal(a, b)


def test_buffer_placement_in_a_row_in_a_slot_and_alone():
    """optimization._place, the one rule for where a loop's buffer lives.  In a row of an arena: a zero-filled buffer of the full shape in the
    row, the tensor in its leading corner, at the same offset of every row.  No row, private (a frame slot): a buffer of its own.  Neither:
    the tensor itself when it already has the shape, dtype and contiguity (a loop of one frame aliases the caller's soft masks), a converted
    copy otherwise."""
    from vsrd_amd import optimization
    tensor = torch.arange(1.0, 13.0, dtype=torch.float64).reshape(2, 6)[:, ::2]            # [2, 3], float64, not contiguous, no zeros
    flags = torch.tensor([[1, 0, 1], [1, 1, 1]], dtype=torch.bool)
    arena = optimization.FrameArena(3, 10_000, "cpu")
    arena.buffer.fill_(0xFF)                 # (fresh host memory is usually zero already: the zeros below must be _place's own)
    low, high = arena.buffer.data_ptr(), arena.buffer.data_ptr() + arena.buffer.numel()
    placed = []
    for row in arena.rows:
        full = optimization._place(tensor, (4, 5), torch.float32, row)
        bits = optimization._place(flags, (4, 5), torch.uint8, row)
        same = optimization._place(tensor, (2, 3), torch.float32, row, private=True)      # (a row's loop is persistent: the row decides)
        placed.append((full, bits, same))
        assert full.shape == (4, 5) and full.dtype == torch.float32 and full.is_contiguous() and bits.dtype == torch.uint8
        assert torch.equal(full[:2, :3], tensor.to(torch.float32)) and torch.equal(bits[:2, :3], flags.to(torch.uint8)) and torch.equal(same, tensor.to(torch.float32))
        outside = torch.ones(4, 5, dtype=torch.bool)
        outside[:2, :3] = False
        assert bool((full[outside] == 0).all()) and bool((bits[outside] == 0).all())
        assert all(low <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= high for t in (full, bits, same))
    assert arena.rows[0].layout == arena.rows[1].layout == arena.rows[2].layout and len(arena.rows[0].layout) == 3
    for k in range(3):
        assert placed[1][k].data_ptr() - placed[0][k].data_ptr() == arena.stride and placed[2][k].data_ptr() - placed[0][k].data_ptr() == 2 * arena.stride
    placed[1][0].fill_(9.0)      # rows do not overlap
    assert float(placed[0][0].max()) == float(tensor.max()) == float(placed[2][0].max())
    with pytest.raises(RuntimeError, match="exhausted"):
        optimization._place(tensor, (100, 100), torch.float32, arena.rows[0])

    # a frame slot: a buffer of its own, also for a tensor that would do as it is
    plain = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    own = optimization._place(plain, (2, 3), torch.float32, private=True)
    assert own.data_ptr() != plain.data_ptr() and torch.equal(own, plain)
    own.fill_(-1.0)
    assert torch.equal(plain, torch.arange(6, dtype=torch.float32).reshape(2, 3))
    larger = optimization._place(plain, (3, 4), torch.float32, private=True)
    assert larger.shape == (3, 4) and torch.equal(larger[:2, :3], plain) and float(larger[2:].abs().sum() + larger[:, 3:].abs().sum()) == 0.0

    # a loop of one frame: the caller's tensor itself, or a converted copy
    assert optimization._place(plain, (2, 3), torch.float32).data_ptr() == plain.data_ptr()
    for other in (plain.double(), torch.arange(12, dtype=torch.float32).reshape(2, 6)[:, ::2]):
        converted = optimization._place(other, (2, 3), torch.float32)
        assert converted.data_ptr() != other.data_ptr() and converted.dtype == torch.float32 and converted.is_contiguous()
        assert torch.equal(converted, other.to(torch.float32))
    with pytest.raises(ValueError):
        optimization._place(plain, (3, 4), torch.float32)          # (nothing to lay out for: the capacities are the frame's own counts)


def test_reset_admits_the_loops_shape_or_up_to_its_capacities():
    """optimization._incoming_shape, reset()'s admission check: a frame pack or a FrameInputs of the loop's image size; under a header 1..capacity
    views and instances, without one exactly the loop's own counts; each refusal a ValueError that names the axis and the limit."""
    from vsrd_amd import frames, optimization

    def inputs(v, h, w, n):
        return optimization.FrameInputs((h, w), torch.zeros(v, 3, 3), torch.zeros(v, 4, 4), torch.zeros(v, h, w, n), torch.zeros(v, n, 2, 2),
                                        torch.zeros(v, n, dtype=torch.bool))

    def pack(v, h, w, n):
        import numpy as np
        entries = v * n
        return frames.FramePack((h, w), np.zeros((v, 3, 3), np.float32), np.zeros((v, 4, 4), np.float32), np.arange(v + 1, dtype=np.int64) * n,
                                np.tile(np.arange(n, dtype=np.int64), v), np.zeros(entries + 1, np.int64), np.zeros((0, 2), np.int32),
                                np.zeros((entries, h, (w + 7) // 8), np.uint8))

    loop, capacities = (2, 4, 6, 3), (3, 5)
    for make in (inputs, pack):
        for v in (1, 2, 3):
            for n in (1, 3, 5):
                assert optimization._incoming_shape(make(v, 4, 6, n), loop, capacities) == (v, 4, 6, n)
        for refused, word in (((0, 4, 6, 3), r"1\.\.3 views, got 0"), ((4, 4, 6, 3), r"1\.\.3 views, got 4"), ((2, 4, 6, 0), r"1\.\.5 instances, got 0"),
                              ((2, 4, 6, 6), r"1\.\.5 instances, got 6"), ((2, 4, 8, 3), "image size"), ((2, 5, 6, 3), "image size")):
            with pytest.raises(ValueError, match=word):
                optimization._incoming_shape(make(*refused), loop, capacities)
        # without a header: the loop's own shape and nothing else
        assert optimization._incoming_shape(make(*loop), loop) == loop
        for refused, word in (((1, 4, 6, 3), r"2\.\.2 views, got 1"), ((3, 4, 6, 3), r"2\.\.2 views, got 3"), ((2, 4, 6, 2), r"3\.\.3 instances, got 2"),
                              ((2, 4, 6, 4), r"3\.\.3 instances, got 4"), ((2, 4, 8, 3), "image size")):
            with pytest.raises(ValueError, match=word):
                optimization._incoming_shape(make(*refused), loop)
    wrong = inputs(2, 4, 6, 3)
    wrong.image_size = (4, 8)            # a FrameInputs whose image_size is not its soft masks'
    with pytest.raises(ValueError, match="image_size"):
        optimization._incoming_shape(wrong, loop, capacities)


def test_frame_output_buffer_lists_and_their_rows():
    """The buffers the five outputs create at first use (optimization._OUTPUTS[...].buffers: plain functions of the capacities and the image
    size; `V`: the view capacity, for group_labels the label-view capacity), against literals: names, shapes, dtypes, fills and order; what
    the ONE table says of each beyond them; and the rows they give in an arena, in two orders of first use -- equal in both rows, at the
    offsets 256-byte alignment gives."""
    from vsrd_amd import optimization
    V, N, H, W = 3, 5, 6, 9
    f32, u8, nan = torch.float32, torch.uint8, float("nan")
    want = dict(labels=[("camera_corners", (V, N, 8, 3), f32, 0.0), ("boxes_2d", (V, N, 4), f32, 0.0), ("mean_iou", (N, N), f32, 0.0),
                        ("matched_gt", (N,), torch.int64, 0), ("confidences", (N,), f32, 0.0)],
                masks=[("inside", (N, H, 2), torch.uint8, 0), ("soft", (H * W, N), f32, 0.0), ("counts", (N, 3), torch.int32, 0)],
                metrics=[("gt_boxes_3d", (N, 8, 3), f32, nan), ("rectification", (3, 3), f32, 0.0), ("corners", (N, 8, 3), f32, 0.0),
                         ("ious", (N, 2), f32, nan), ("summary", (8,), f32, 0.0)],
                group_labels=[("count", (1,), torch.int32, 1), ("frame_ids", (V,), torch.int64, -1), ("extrinsics", (V, 16), f32, 0.0),
                              ("intrinsics", (V, 9), f32, 0.0), ("gt_boxes", (V, N, 4), f32, 0.0), ("visible", (V, N), u8, 0),
                              ("camera_corners", (V, N, 8, 3), f32, 0.0), ("boxes_2d", (V, N, 4), f32, 0.0), ("mean_iou", (N, N), f32, 0.0),
                              ("matched_gt", (N,), torch.int64, 0), ("confidences", (N,), f32, 0.0)],
                surface=[("light", (3,), f32, 0.0), ("palette", (N, 3), f32, 0.0), ("background", (H * W, 3), u8, 0), ("converged_bits", (H, 2), u8, 0),
                         ("shadow_bits", (H, 2), u8, 0), ("instance", (H * W,), u8, 255), ("range", (H * W,), f32, 0.0), ("colors", (H * W, 3), u8, 0)])
    assert list(optimization._OUTPUTS) == ["labels", "masks", "metrics", "group_labels", "surface"] == list(want)
    assert not any(hasattr(optimization, gone) for gone in ("_LABEL_VIEW_OUTPUTS", "_IMAGE_OUTPUTS", "_output"))
    # what differs between them, as data: what they read of the last step, which capacity leads their buffers, which rows hold them
    table = optimization._OUTPUTS
    assert [table[name].last_step for name in want] == [None, "field block", "matching", None, "field block"]
    assert [table[name].leading for name in want] == ["view_capacity"] * 3 + ["label_view_capacity", "view_capacity"]
    for label_views in (0, 1, 7):
        for surface in (False, True):
            switches = dict(label_views=label_views, headed=False, photometric=False, surface=surface)
            assert [bool(table[name].held(switches)) for name in want] == [True, True, True, label_views > 0, surface]
    for name, buffers in want.items():
        got = optimization._OUTPUTS[name].buffers(V, N, H, W)
        assert [(key, tuple(shape), dtype) for key, shape, dtype, _ in got] == [(key, shape, dtype) for key, shape, dtype, _ in buffers], name
        assert all(fill == expected or fill != fill and expected != expected for (*_, fill), (*_, expected) in zip(got, buffers)), name
    item = {f32: 4, torch.int64: 8, torch.int32: 4, torch.uint8: 1}
    for order in (("labels", "masks", "metrics"), ("metrics", "masks", "labels"), tuple(want), tuple(want)[::-1]):
        arena = optimization.FrameArena(2, 20_000, "cpu")
        layout, cursor = [], 0
        for name in order:
            for _, shape, dtype, _ in want[name]:
                nbytes = item[dtype] * functools.reduce(lambda a, b: a * b, shape)
                layout.append((cursor, nbytes))
                cursor = (cursor + nbytes + 255) // 256 * 256
        for row in arena.rows:
            for name in order:
                for key, shape, dtype, fill in optimization._OUTPUTS[name].buffers(V, N, H, W):
                    tensor = row.new(shape, dtype, fill)
                    assert tensor.shape == tuple(shape) and tensor.dtype == dtype
                    assert bool(torch.isnan(tensor).all() if fill != fill else (tensor == fill).all()), (name, key)
        assert arena.rows[0].layout == arena.rows[1].layout == layout, order


ROW_SHAPES = ((2, 16, 72, 3), (17, 376, 1408, 8))
# FrameBatch._row_bytes as recorded BEFORE the outputs shared one table, per shape over label_views in (0, 2) x headed x photometric x surface x log
# (itertools.product, each off then on): the defaults of OptimizationConfig with loss_weights["photometric_loss"] = 0.1, the log at intervals 50 / 500
ROW_BYTES = (
    230352384, 246781440, 230366464, 246795520, 451705344, 468134400, 451719424, 468148480,
    230352640, 246781696, 230366720, 246795776, 451705600, 468134656, 451719680, 468148736,
    230355712, 246784768, 230369792, 246798848, 451708672, 468137728, 451722752, 468151808,
    230355968, 246785024, 230370048, 246799104, 451708928, 468137984, 451723008, 468152064,
    1188851200, 1205312000, 1194807808, 1211268608, 1825562112, 1842022912, 1831518720, 1847979520,
    1188851456, 1205312256, 1194808064, 1211268864, 1825562368, 1842023168, 1831518976, 1847979776,
    1188855296, 1205316096, 1194811904, 1211272704, 1825566208, 1842027008, 1831522816, 1847983616,
    1188855552, 1205316352, 1194812160, 1211272960, 1825566464, 1842027264, 1831523072, 1847983872)


def _row_grid():
    import dataclasses
    import itertools
    from vsrd_amd import losses, optimization
    base = optimization.OptimizationConfig(loss_weights={**losses.LOSS_WEIGHTS, "photometric_loss": 0.1})
    logged = dataclasses.replace(base, scalar_interval=50, checkpoint_interval=500)
    for shape in ROW_SHAPES:
        for label_views, headed, photometric, surface, log in itertools.product((0, 2), (False, True), (False, True), (False, True), (False, True)):
            yield shape, logged if log else base, dict(label_views=label_views, headed=headed, photometric=photometric, surface=surface)


def test_row_sizes_are_what_they_were_before_the_one_table(lib):
    """FrameBatch._row_bytes over the grid of its switches, against the values recorded on the commit before: one loop over one table counts
    what three loops over three tables counted."""
    from vsrd_amd import optimization
    got = [optimization.FrameBatch._row_bytes(shape, config, **switches) for shape, config, switches in _row_grid()]
    assert len(got) == len(ROW_BYTES) == 64 and tuple(got) == ROW_BYTES
    # rows without surface=True, and rows without label views, are as large as they were: the switch alone moves the size, by the buffers' own
    aligned = optimization.FrameArena.aligned
    for (shape, config, switches), size in zip(_row_grid(), got):
        V, H, W, N = shape
        for name, off in (("surface", dict(surface=False)), ("group_labels", dict(label_views=0))):
            leading = switches["label_views"] if name == "group_labels" else V
            own = sum(aligned(optimization._buffer_bytes(s, d)) for _, s, d, _ in optimization._OUTPUTS[name].buffers(leading, N, H, W))
            held = switches["surface"] if name == "surface" else switches["label_views"] > 0
            assert size - optimization.FrameBatch._row_bytes(shape, config, **dict(switches, **off)) == (own if held else 0), (shape, switches, name)


def test_a_sixth_output_is_counted_under_its_own_row_switch(lib, monkeypatch):
    """An entry put into the table with a row switch of its own: FrameBatch._row_bytes counts its buffers exactly under that switch, laid out
    for the capacity it names -- no line of FrameOptimizer or FrameBatch knows its name."""
    import dataclasses
    from vsrd_amd import optimization

    def buffers(V, N, H, W):
        return [("planes", (V, H, W), torch.float32, 0.0), ("flags", (N, 3), torch.uint8, 0)]

    stand_in = dataclasses.replace(optimization._OUTPUTS["labels"], buffers=buffers, leading="label_view_capacity",
                                   held=lambda switches: switches["headed"] and not switches["surface"])
    plain = {case: optimization.FrameBatch._row_bytes(shape, config, **switches) for case, (shape, config, switches) in enumerate(_row_grid())}
    monkeypatch.setitem(optimization._OUTPUTS, "stand_in", stand_in)
    assert list(optimization._OUTPUTS)[-1] == "stand_in" and len(optimization._OUTPUTS) == 6
    aligned, counted = optimization.FrameArena.aligned, 0
    for case, (shape, config, switches) in enumerate(_row_grid()):
        V, H, W, N = shape
        extra = aligned(switches["label_views"] * H * W * 4) + aligned(N * 3) if switches["headed"] and not switches["surface"] else 0
        assert optimization.FrameBatch._row_bytes(shape, config, **switches) - plain[case] == extra, (shape, switches)
        counted += extra > 0
    assert counted == 16             # (headed, no surface: a quarter of the grid; with label_views = 0 the planes are empty and the flags remain)


class _StandInSource:
    """What the launcher's `_collect` asks of a loop (`active` None) or a batch: labels / group_labels / masks / surface / metrics of the
    documented shapes, on the host; `surface_calls`: what surface() was asked with."""

    def __init__(self, counts, summaries, boxes_3d="given"):
        self.counts, self.summaries, self.asked, self.surface_calls = counts, summaries, [], []
        self.inputs = type("Inputs", (), dict(boxes_3d=None if boxes_3d is None else torch.zeros(counts[0], 8, 3)))()

    def _answer(self, name, active, make):
        self.asked.append(name)
        return make(0) if active is None else [make(f) for f in range(active)]

    def _labels_of(self, f):
        n = self.counts[f]
        corners = torch.tensor([[0., 0, 0], [1, 0, 0], [1, 0, 2], [0, 0, 2], [0, 1, 0], [1, 1, 0], [1, 1, 2], [0, 1, 2]]) + torch.tensor([0.0, 0.0, 10.0 + f])
        return dict(boxes_3d=corners.expand(1, n, 8, 3).clone(), boxes_2d=torch.tensor([[10.0, 20.0], [30.0, 40.0]]).expand(1, n, 2, 2).clone(),
                    confidences=torch.full((n,), 0.5), matched_gt=torch.arange(n), mean_iou=torch.eye(n))

    def labels(self, active=None):
        return self._answer("labels", active, self._labels_of)

    def group_labels(self, active=None):       # (a group of one frame, id 40 + f)
        return self._answer("group_labels", active, lambda f: dict(self._labels_of(f), frame_ids=torch.tensor([40 + f])))

    def surface(self, active=None, light=None, background=None):
        self.surface_calls.append(dict(active=active, light=light, background=background))
        return self._answer("surface", active, lambda f: dict(
            converged_bits=torch.zeros(4, 2, dtype=torch.uint8), shadow_bits=torch.zeros(4, 2, dtype=torch.uint8), instance=torch.full((4, 9), 255, dtype=torch.uint8),
            range=torch.zeros(4, 9), colors=torch.full((4, 9, 3), 10 * (f + 1), dtype=torch.uint8), light=torch.tensor([0.0, 1.0, 0.0]), shape=(4, 9), view=0, hard=True))

    def masks(self, active=None):
        def make(f):
            n = self.counts[f]
            return dict(inside=torch.zeros(n, 4, 2, dtype=torch.uint8), counts=torch.ones(n, 3, dtype=torch.int32), mask_iou=torch.full((n,), 0.25 * (f + 1)),
                        threshold=0.5, shape=(4, 9), soft=torch.zeros(4, 9, n))
        return self._answer("masks", active, make)

    def metrics(self, active=None):
        return self._answer("metrics", active, lambda f: dict(summary=torch.tensor(self.summaries[f]), iou_3d=torch.zeros(self.counts[f])))


def _render_work(out, **flags):
    import argparse
    from vsrd_amd import launcher
    args = argparse.Namespace(num_steps=3, warmup_steps=1, rays=8, samples=8, fp32_mlp=False, adjoint_item_slots=0,
                              **dict(dict(predictions=False, masks=False, metrics=False), **flags))
    work = launcher._RenderWork(args, dict(out=str(out), seed=0), "cpu", None)
    work._begin_outputs()
    return work


def test_launcher_collects_and_writes_a_frames_outputs_in_one_place(tmp_path):
    """launcher._RenderWork._collect / _write_outputs on stand-in sources: one loop, and a batch of two."""
    from vsrd_amd import formats
    summary, empty = [2.0, 0.5, 0.75, 1.0, 1.0, 0.5, 1.0, 0.0], [0.0] * 8
    files = ("predictions/view_00.json", "labels/view_00.txt", "masks/view_00.npz")

    def folder(work, frame):
        return os.path.dirname(work.path_of(frame))
    # ---- one loop, every flag ----
    work = _render_work(tmp_path / "loop", predictions=True, masks=True, metrics=True)
    assert set(work.phase_seconds) == {"labels", "labels_write", "masks", "masks_write", "metrics"}
    loop, payloads = _StandInSource([3], [summary]), [dict(metrics={})]
    pending = work._collect(loop, [(7, work.path_of(7))], payloads)
    assert loop.asked == ["labels", "masks", "metrics"] and len(pending) == 2 and not os.path.exists(folder(work, 7))
    assert work.phase_seconds["labels_write"] == 0.0 and work.phase_seconds["masks_write"] == 0.0
    work._write_outputs(pending)
    assert all(os.path.exists(os.path.join(folder(work, 7), name)) for name in files) and not os.path.exists(work.path_of(7))    # (before any checkpoint)
    assert set(payloads[0]["metrics"]) == {"mask_iou", *formats.FRAME_METRIC_NAMES} and payloads[0]["metrics"]["mask_iou"] == 0.25
    assert work.frame_metrics == {7: formats.frame_metrics(summary)} and work.frame_metrics[7]["iou_bev"] == 0.75
    assert all(work.phase_seconds[key] > 0.0 for key in ("labels", "labels_write", "masks", "masks_write", "metrics"))
    assert "soft" not in formats.load_frame_masks(folder(work, 7)) and formats.load_frame_masks(folder(work, 7))["shape"] == (4, 9)
    # ---- a loop whose frame has no 3-D ground truth is never asked for metrics ----
    work = _render_work(tmp_path / "bare", masks=True, metrics=True)
    assert set(work.phase_seconds) == {"masks", "masks_write", "metrics"}
    bare, payloads = _StandInSource([3], [summary], boxes_3d=None), [dict(metrics={})]
    work._write_outputs(work._collect(bare, [(1, work.path_of(1))], payloads))
    assert bare.asked == ["masks"] and payloads[0]["metrics"] == dict(mask_iou=0.25) and work.frame_metrics == {} and work.phase_seconds["metrics"] == 0.0
    assert os.listdir(folder(work, 1)) == ["masks"]
    # ---- a batch of two: always asked; the member with an all-zero summary is skipped ----
    work = _render_work(tmp_path / "batch", predictions=True, masks=True, metrics=True)
    batch, payloads = _StandInSource([3, 5], [empty, summary], boxes_3d=None), [dict(metrics={}), dict(metrics={})]
    rows = [(4, work.path_of(4)), (9, work.path_of(9))]
    pending = work._collect(batch, rows, payloads, active=2)
    assert batch.asked == ["labels", "masks", "metrics"] and [key for key, *_ in pending] == ["labels_write"] * 2 + ["masks_write"] * 2
    work._write_outputs(pending)
    for frame in (4, 9):
        assert all(os.path.exists(os.path.join(folder(work, frame), name)) for name in files) and not os.path.exists(work.path_of(frame))
    assert payloads[0]["metrics"] == dict(mask_iou=0.25) and set(payloads[1]["metrics"]) == {"mask_iou", *formats.FRAME_METRIC_NAMES}
    assert payloads[1]["metrics"]["mask_iou"] == 0.5 and work.frame_metrics == {9: formats.frame_metrics(summary)}
    # ---- one flag: its keys only; no flag: no clock, nothing asked, nothing written ----
    work = _render_work(tmp_path / "labels", predictions=True)
    only = _StandInSource([2], [summary])
    work._write_outputs(work._collect(only, [(0, work.path_of(0))], [dict(metrics={})]))
    assert set(work.phase_seconds) == {"labels", "labels_write"} and only.asked == ["labels"] and sorted(os.listdir(folder(work, 0))) == ["labels", "predictions"]
    work = _render_work(tmp_path / "none")
    nothing, payloads = _StandInSource([2], [summary]), [dict(metrics={})]
    pending = work._collect(nothing, [(0, work.path_of(0))], payloads)
    work._write_outputs(pending)
    assert work.phase_seconds is None and nothing.asked == [] and pending == [] and payloads == [dict(metrics={})] and not os.path.exists(tmp_path / "none")
    # ---- all five flags: the order of asking, the clock's keys, and what surface() is asked with ----
    every = dict(predictions=True, group_predictions=True, masks=True, surface=True, metrics=True)
    order = ["labels", "group_labels", "masks", "surface", "metrics"]
    more = ("group/predictions/0000000040.json", "group/labels/0000000040.txt", "surface/view_00.npz", "surface/view_00.png")
    work = _render_work(tmp_path / "every", surface_light=(0.0, 0.0, 1.0), **every)
    assert list(work.phase_seconds) == ["labels", "labels_write", "group_labels", "group_labels_write", "masks", "masks_write", "surface", "surface_write", "metrics"]
    photograph = torch.full((4, 9, 3), 7, dtype=torch.uint8)
    work.backgrounds[7] = photograph
    loop, payloads = _StandInSource([3], [summary]), [dict(metrics={})]
    pending = work._collect(loop, [(7, work.path_of(7))], payloads)
    assert loop.asked == order and [key for key, *_ in pending] == ["labels_write", "group_labels_write", "masks_write", "surface_write"]
    assert len(loop.surface_calls) == 1 and loop.surface_calls[0]["active"] is None and loop.surface_calls[0]["light"] == (0.0, 0.0, 1.0)
    assert loop.surface_calls[0]["background"] is photograph and work.backgrounds == {}
    work._write_outputs(pending)
    assert all(os.path.exists(os.path.join(folder(work, 7), name)) for name in files + more) and all(value > 0.0 for value in work.phase_seconds.values())
    assert set(payloads[0]["metrics"]) == {"mask_iou", *formats.FRAME_METRIC_NAMES}
    # a loop without a photograph, and one without a light: asked with None
    loop = _StandInSource([3], [summary])
    _render_work(tmp_path / "dark", **every)._collect(loop, [(7, work.path_of(7))], [dict(metrics={})])
    assert loop.asked == order and loop.surface_calls == [dict(active=None, light=None, background=None)]
    # a batch: its frames' photographs in order -- or, when not EVERY frame of the group carries one, none at all (and none is left behind)
    for carried, expected in (((4, 9), "both"), ((9,), None), ((), None)):
        work = _render_work(tmp_path / f"batch_{len(carried)}", **every)
        work.backgrounds.update({frame: torch.full((4, 9, 3), frame, dtype=torch.uint8) for frame in carried})
        kept = dict(work.backgrounds)
        batch, payloads = _StandInSource([3, 5], [empty, summary], boxes_3d=None), [dict(metrics={}), dict(metrics={})]
        pending = work._collect(batch, rows, payloads, active=2)
        assert batch.asked == order and len(batch.surface_calls) == 1 and batch.surface_calls[0]["active"] == 2 and work.backgrounds == {}
        background = batch.surface_calls[0]["background"]
        assert background is None if expected is None else len(background) == 2 and background[0] is kept[4] and background[1] is kept[9]
        assert [key for key, *_ in pending] == ["labels_write"] * 2 + ["group_labels_write"] * 2 + ["masks_write"] * 2 + ["surface_write"] * 2
        assert set(work.phase_seconds) == {"labels", "labels_write", "group_labels", "group_labels_write", "masks", "masks_write", "surface", "surface_write", "metrics"}
