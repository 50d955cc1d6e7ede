"""ctypes binding of libvsrd_hip.so (include/vsrd_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is no CPU
fallback: if the shared object is missing, or a tensor is not on a HIP device, every entry
point raises.
"""
import ctypes
import os
import re
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# VSRD_HIP_LIBRARY: an experiment build of the same ABI (tools/phase_timers.py, A/B macros); the product path is the in-tree default
LIBRARY_PATH = os.environ.get("VSRD_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libvsrd_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vsrd_hip.h")

ABI_VERSION = 12
MAX_INSTANCES = 64
MAX_SAMPLES = 256
INSTANCE_STRIDE = 16
MLP_WEIGHTS = 1617
FLAG_FINE_UNIFORMS_SORTED = 1
FLAG_SKIP_EXACT_MISSES = 2
FLAG_NO_CULLING = 4
FLAG_MLP_WEIGHTS_CENTRED = 8
FLAG_RUNNING_MINIMUM = 16
FLAG_GENERAL_ROTATIONS = 32
FLAG_RESIDUAL_SINGLE_KERNEL = 64
FLAG_RESIDUAL_WAVE_PER_RAY = 128
FLAG_STEP_WAVE_PER_RAY = 256
FLAG_STEP_SPLIT_RAY = 512
FLAG_YAW_GRADIENTS = 1024
FLAG_MLP_SPLIT_BF16 = 2048

c_float_p = ctypes.c_void_p  # device pointers travel as integers


class VsrdHipError(RuntimeError):
    pass


class Field(ctypes.Structure):
    _fields_ = [
        ("num_instances", ctypes.c_int32),
        ("temperature", ctypes.c_float),
        ("instances", ctypes.c_void_p),
        ("mlp_weights", ctypes.c_void_p),
    ]


class RenderConfig(ctypes.Structure):
    _fields_ = [
        ("num_rays", ctypes.c_int32),
        ("num_samples", ctypes.c_int32),
        ("distance_near", ctypes.c_float),
        ("distance_far", ctypes.c_float),
        ("sdf_std_deviation", ctypes.c_float),
        ("cosine_ratio", ctypes.c_float),
        ("epsilon", ctypes.c_float),
        ("origin_stride", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("stream_offset", ctypes.c_uint64),
        ("flags", ctypes.c_uint32),
        ("device_schedule", ctypes.c_void_p),
        ("device_stream_offset", ctypes.c_void_p),
        ("ray_indices", ctypes.c_void_p),
        ("rays_per_origin", ctypes.c_int32),
        ("target_columns", ctypes.c_void_p),
        ("target_stride", ctypes.c_int32),
        ("out_distances", ctypes.c_void_p),
        ("out_coarse_weights", ctypes.c_void_p),
        ("out_u_coarse", ctypes.c_void_p),
        ("out_u_fine", ctypes.c_void_p),
        ("num_frames", ctypes.c_int32),          # frame batch (ABI 8): 0 or 1 = one frame
        ("frame_stride", ctypes.c_int64),        # bytes between the frames' copies of every buffer of the call
        ("adjoint_slots_per_item", ctypes.c_int32),   # vsrd_render_residual_step: slots per work item of the MLP adjoint (0: planned)
    ]


class FrameConfig(ctypes.Structure):
    _fields_ = [
        ("num_boxes", ctypes.c_int32),
        ("num_views", ctypes.c_int32),
        ("height", ctypes.c_float),
        ("width", ctypes.c_float),
        ("epsilon", ctypes.c_float),
        ("location_lo", ctypes.c_float * 3),
        ("location_hi", ctypes.c_float * 3),
        ("dimension_lo", ctypes.c_float * 3),
        ("dimension_hi", ctypes.c_float * 3),
        ("num_steps", ctypes.c_int32),
        ("max_temperature", ctypes.c_float),
        ("min_temperature", ctypes.c_float),
        ("max_std", ctypes.c_float),
        ("min_std", ctypes.c_float),
        ("weight_iou", ctypes.c_float),
        ("weight_l1", ctypes.c_float),
        ("weight_silhouette", ctypes.c_float),
        ("beta1", ctypes.c_float),
        ("beta2", ctypes.c_float),
        ("adam_epsilon", ctypes.c_float),
        ("lr_gamma", ctypes.c_float),
        ("num_frames", ctypes.c_int32),
        ("frame_stride", ctypes.c_int64),
    ]


class AdamTensors(ctypes.Structure):
    _fields_ = [
        ("parameter", ctypes.c_void_p),
        ("exp_avg", ctypes.c_void_p),
        ("exp_avg_sq", ctypes.c_void_p),
        ("step", ctypes.c_void_p),
        ("learning_rate", ctypes.c_void_p),
    ]


HYPER_LAYERS = 5


class Hypernetwork(ctypes.Structure):
    _fields_ = [
        ("num_instances", ctypes.c_int32),
        ("num_outputs", ctypes.c_int32),
        ("beta1", ctypes.c_float),
        ("beta2", ctypes.c_float),
        ("adam_epsilon", ctypes.c_float),
        ("lr_gamma", ctypes.c_float),
        ("embeddings", AdamTensors),
        ("weight_v", AdamTensors * HYPER_LAYERS),
        ("weight_g", AdamTensors * HYPER_LAYERS),
        ("bias", AdamTensors * HYPER_LAYERS),
        ("norm_weight", AdamTensors * (HYPER_LAYERS - 1)),
        ("norm_bias", AdamTensors * (HYPER_LAYERS - 1)),
        ("num_frames", ctypes.c_int32),
        ("frame_stride", ctypes.c_int64),
    ]


class FrameHeader(ctypes.Structure):
    """include/vsrd_hip.h::vsrd_frame_header (ABI 9, mixed batches): one frame's own instance count and silhouette normaliser; ABI 12:
    its own view count and the count of its sampling table, read when num_instances carries FRAME_HEADER_HAS_VIEWS."""
    _fields_ = [
        ("num_instances", ctypes.c_int32),
        ("loss_scale", ctypes.c_float),
        ("num_views", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("num_pixels", ctypes.c_int64),
    ]


class FrameMasksConfig(ctypes.Structure):
    """include/vsrd_hip.h::vsrd_frame_masks_config (added within ABI 12): the view, the image size, the sphere-tracing constants and the
    threshold of one vsrd_frame_masks call."""
    _fields_ = [
        ("view", ctypes.c_int32),
        ("num_views", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("num_iterations", ctypes.c_int32),
        ("convergence_criteria", ctypes.c_float),
        ("bounding_radius", ctypes.c_float),
        ("threshold", ctypes.c_float),
        ("target_stride", ctypes.c_int32),
    ]


FRAME_SURFACE_HARD_UNION = 1   # VSRD_SURFACE_*: flags of a vsrd_frame_surface call
FRAME_SURFACE_SHADOWS = 2


class FrameSurfaceConfig(ctypes.Structure):
    """include/vsrd_hip.h::vsrd_frame_surface_config (added within ABI 12): the view, the image size, the sphere-tracing constants, the shadow
    ray's offset, the blend and the light and material colours of one vsrd_frame_surface call."""
    _fields_ = [
        ("view", ctypes.c_int32),
        ("num_views", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("num_iterations", ctypes.c_int32),
        ("convergence_criteria", ctypes.c_float),
        ("bounding_radius", ctypes.c_float),
        ("shadow_offset", ctypes.c_float),
        ("flags", ctypes.c_uint32),
        ("background_pixels", ctypes.c_int32),
        ("alpha", ctypes.c_float),
        ("shininess", ctypes.c_float),
        ("background_color", ctypes.c_float * 3),
        ("light_ambient", ctypes.c_float * 3),
        ("light_diffuse", ctypes.c_float * 3),
        ("light_specular", ctypes.c_float * 3),
        ("material_ambient", ctypes.c_float * 3),
        ("material_specular", ctypes.c_float * 3),
        ("material_emission", ctypes.c_float * 3),
    ]


class LogSegment(ctypes.Structure):
    """include/vsrd_hip.h::vsrd_log_segment (device memory): `count` 32-bit words from `source` to word `offset` of a snapshot slot."""
    _fields_ = [
        ("source", ctypes.c_void_p),
        ("count", ctypes.c_int64),
        ("offset", ctypes.c_int64),
    ]


class FrameLogConfig(ctypes.Structure):
    """include/vsrd_hip.h::vsrd_frame_log_config (added within ABI 12): the intervals, capacities and device buffers of one vsrd_frame_log call."""
    _fields_ = [
        ("scalar_interval", ctypes.c_int32),
        ("checkpoint_interval", ctypes.c_int32),
        ("history_capacity", ctypes.c_int32),
        ("snapshot_capacity", ctypes.c_int32),
        ("snapshot_floats", ctypes.c_int64),
        ("num_segments", ctypes.c_int32),
        ("num_frames", ctypes.c_int32),
        ("frame_stride", ctypes.c_int64),
        ("step", ctypes.c_void_p),
        ("record", ctypes.c_void_p),
        ("learning_rates", ctypes.c_void_p),
        ("schedule", ctypes.c_void_p),
        ("summary", ctypes.c_void_p),
        ("segments", ctypes.c_void_p),
        ("history", ctypes.c_void_p),
        ("snapshots", ctypes.c_void_p),
        ("snapshot_steps", ctypes.c_void_p),
        ("counters", ctypes.c_void_p),
    ]


class PatchCorrelationConfig(ctypes.Structure):
    """include/vsrd_hip.h::vsrd_patch_correlation_config (added within ABI 12): the shape and the two epsilons of one
    vsrd_patch_correlation_forward / _backward call."""
    _fields_ = [
        ("num_views", ctypes.c_int32),
        ("num_rays", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("patch_width", ctypes.c_int32),
        ("patch_height", ctypes.c_int32),
        ("top_k", ctypes.c_int32),
        ("target_view", ctypes.c_int32),
        ("sample_epsilon", ctypes.c_float),
        ("correlation_epsilon", ctypes.c_float),
    ]


class FramePhotometricConfig(ctypes.Structure):
    """include/vsrd_hip.h::vsrd_frame_photometric_config (added within ABI 12): the trace's constants, the term's weight relative to the
    silhouette term and the batch fields of one vsrd_frame_photometric call."""
    _fields_ = [
        ("num_iterations", ctypes.c_int32),
        ("convergence_criteria", ctypes.c_float),
        ("bounding_radius", ctypes.c_float),
        ("scale", ctypes.c_float),
        ("num_frames", ctypes.c_int32),
        ("frame_stride", ctypes.c_int64),
    ]


PHOTOMETRIC_RAYS = 2048        # VSRD_PHOTOMETRIC_MAX_RAYS: the rays of one vsrd_frame_photometric call (the table sampler's limit)
PATCH_VIEWS = 32              # VSRD_PATCH_MAX_VIEWS: the limits of vsrd_patch_correlation_forward / _backward
PATCH_PIXELS = 256             # VSRD_PATCH_MAX_PIXELS
PATCH_RAYS = 65535             # VSRD_PATCH_MAX_RAYS
FRAME_LOG_COLUMNS = 22        # VSRD_LOG_SCALARS: (step | record 5 | learning rates 5 | schedule 3 | metrics summary 8) of a history row
FRAME_LOG_SEGMENTS = 32        # VSRD_LOG_MAX_SEGMENTS: entries of a frame's snapshot table
FRAME_HEADER_HAS_VIEWS = 0x10000
MAX_VIEWS = 32                 # the frame glue's limit (csrc/host_checks.h: kFrameMaxViews)
MAX_LABEL_VIEWS = 4096         # VSRD_MAX_LABEL_VIEWS: the label views (a frame's group) of vsrd_frame_group_labels


_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
            "size_t": ctypes.c_size_t}
_RETURNS = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
# host structures, passed as const T*; every other pointer is device memory (vsrd_frame_header too) or the stream, and travels as an integer
_HOST_STRUCTS = {"vsrd_field": Field, "vsrd_render_config": RenderConfig, "vsrd_frame_config": FrameConfig, "vsrd_adam_tensors": AdamTensors,
                 "vsrd_hypernetwork": Hypernetwork, "vsrd_frame_masks_config": FrameMasksConfig, "vsrd_frame_surface_config": FrameSurfaceConfig,
                 "vsrd_frame_log_config": FrameLogConfig,
                 "vsrd_patch_correlation_config": PatchCorrelationConfig, "vsrd_frame_photometric_config": FramePhotometricConfig}
_DEVICE_POINTEES = {"void", "float", "uint8_t", "int32_t", "int64_t", "uint64_t", "vsrd_frame_header"}


def _argtype(parameter):
    """One parameter of a prototype ("const float* origins", "size_t workspace_bytes") -> its ctypes type.  A type the binding does not know
    is an error, never a guess."""
    match = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*\w+", parameter.strip())
    if match:
        const, name, star = match.groups()
        if not star and not const and name in _SCALARS:
            return _SCALARS[name]
        if star and const and name in _HOST_STRUCTS:
            return ctypes.POINTER(_HOST_STRUCTS[name])
        if star and name in _DEVICE_POINTEES:
            return ctypes.c_void_p
    raise VsrdHipError(f"{HEADER_PATH}: no ctypes type for the parameter {parameter.strip()!r}")


def _signatures():
    """symbol -> (restype, argtypes), read from the prototypes of include/vsrd_hip.h: the header is the one place a prototype is written."""
    if not os.path.exists(HEADER_PATH):
        raise VsrdHipError(f"{HEADER_PATH} not found: the ctypes binding is derived from the header's prototypes")
    with open(HEADER_PATH) as file:
        text = re.sub(r"/\*.*?\*/", "", file.read(), flags=re.S)
    table = {}
    for restype, name, parameters in re.findall(r"^(int32_t|size_t|const char\*)\s+(vsrd_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        table[name] = (_RETURNS[restype], [] if parameters.strip() == "void" else [_argtype(p) for p in parameters.split(",")])
    return table


SIGNATURES = _signatures()

E_INVALID_ARGUMENT, E_UNSUPPORTED, E_LAUNCH, E_WORKSPACE = -1, -2, -3, -4      # include/vsrd_hip.h: VSRD_E_*

_lock = threading.Lock()
_lib = None


def load():
    """Load (once) and return the ctypes handle.  Raises if the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIBRARY_PATH):
                raise VsrdHipError(
                    f"{LIBRARY_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(hipcc --offload-arch=gfx950).  vsrd_amd has no CPU fallback.")
            lib = ctypes.CDLL(LIBRARY_PATH)
            for name, (restype, argtypes) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = restype
                fn.argtypes = argtypes
            if lib.vsrd_abi_version() != ABI_VERSION:
                raise VsrdHipError(f"ABI mismatch: library {lib.vsrd_abi_version()} vs binding {ABI_VERSION}")
            _lib = lib
    return _lib


def check(code):
    if code != 0:
        raise VsrdHipError(f"libvsrd_hip: {load().vsrd_error_string(code).decode()} (code {code})")


def ptr(tensor):
    """Device pointer of a contiguous fp32 HIP tensor (None -> NULL)."""
    if tensor is None:
        return None
    if not tensor.is_cuda:
        raise VsrdHipError("vsrd_amd operates on HIP device tensors only (got a CPU tensor); there is no CPU fallback")
    if tensor.dtype != torch.float32:
        raise VsrdHipError(f"expected float32, got {tensor.dtype}")
    if not tensor.is_contiguous():
        raise VsrdHipError("internal error: non-contiguous tensor handed to the C ABI")
    return ctypes.c_void_p(tensor.data_ptr())


def iptr(tensor):
    """Device pointer of a contiguous int32 HIP tensor."""
    if not tensor.is_cuda or tensor.dtype != torch.int32 or not tensor.is_contiguous():
        raise VsrdHipError("expected a contiguous int32 HIP tensor")
    return ctypes.c_void_p(tensor.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_field(instances, temperature, mlp_weights=None):
    return Field(int(instances.shape[0]), float(temperature), ptr(instances).value,
                 None if mlp_weights is None else ptr(mlp_weights).value)


def make_frame_config(num_boxes, num_views, image_size, epsilon, location_range, dimension_range, num_steps=0, temperatures=(0.0, 0.0),
                      std_deviations=(0.0, 0.0), loss_weights=(0.0, 0.0, 0.0), betas=(0.0, 0.0), adam_epsilon=0.0, lr_gamma=0.0, frames=None):
    """include/vsrd_hip.h::vsrd_frame_config.  `image_size` (height, width); `location_range` / `dimension_range` [2][3] = (lo, hi);
    `temperatures` / `std_deviations` (max, min); `loss_weights` (iou, l1, silhouette); `frames`: optional (num_frames, frame_stride in
    bytes).  What only the prologues and the epilogue read (from `num_steps` on) defaults to zero, as in a fresh FrameConfig."""
    vec3 = lambda row: (ctypes.c_float * 3)(*(float(row[j]) for j in range(3)))
    return FrameConfig(int(num_boxes), int(num_views), float(image_size[0]), float(image_size[1]), float(epsilon),
                       vec3(location_range[0]), vec3(location_range[1]), vec3(dimension_range[0]), vec3(dimension_range[1]),
                       int(num_steps), *map(float, temperatures), *map(float, std_deviations), *map(float, loss_weights), *map(float, betas),
                       float(adam_epsilon), float(lr_gamma), *((0, 0) if frames is None else (int(frames[0]), int(frames[1]))))


def make_config(num_rays, num_samples, distance_range, sdf_std_deviation, cosine_ratio, epsilon, origin_stride,
                seed=0, stream_offset=0, flags=0, schedule=None, gather=None, samples=None, frames=None, adjoint_slots_per_item=0):
    """`schedule`: optional device tensor float32 [3] = (temperature, sdf_std_deviation, cosine_ratio) read by the kernels at
    start instead of the by-value scalars; `stream_offset` may likewise be a device int64 tensor (hipGraph replay).
    `samples`: optional (distances [R,2S], coarse_weights [R,S-1], u_coarse [R,S], u_fine [R,S]) float32 device tensors (any may be None)
    that vsrd_render_silhouette_step fills with its own state between the passes (vsrd_render_config::out_*).
    `frames`: optional (num_frames, frame_stride in bytes) -- a batch of independent frames in one launch (include/vsrd_hip.h, ABI 8)."""
    schedule_ptr = offset_ptr = None
    if schedule is not None:
        if schedule.dtype != torch.float32 or schedule.numel() != 3 or not schedule.is_cuda or not schedule.is_contiguous():
            raise ValueError("schedule must be a contiguous float32 device tensor of 3 elements")
        schedule_ptr = schedule.data_ptr()
    if isinstance(stream_offset, torch.Tensor):
        if stream_offset.dtype != torch.int64 or stream_offset.numel() != 1 or not stream_offset.is_cuda:
            raise ValueError("a tensor stream_offset must be a device int64 scalar")
        offset_ptr, stream_offset = stream_offset.data_ptr(), 0
    ray_indices = target_columns = None
    rays_per_origin = target_stride = 0
    if gather is not None:        # (ray_indices int64 [R] or None, rays_per_origin, target_columns int32 [N] or None, target_stride): vsrd_render_config gather
        indices, rays_per_origin, columns, target_stride = gather
        if indices is not None:   # (None: a dense launch that only maps the target columns)
            if indices.dtype != torch.int64 or not indices.is_cuda or not indices.is_contiguous() or indices.numel() != int(num_rays):
                raise ValueError("ray_indices must be a contiguous int64 device tensor with one entry per ray")
            ray_indices = indices.data_ptr()
        if columns is not None:
            target_columns = iptr(columns).value
    outs = [None, None, None, None]
    if samples is not None:
        outs = [None if t is None else ptr(t).value for t in samples]
    return RenderConfig(int(num_rays), int(num_samples), float(distance_range[0]), float(distance_range[1]),
                        float(sdf_std_deviation), float(cosine_ratio), float(epsilon), int(origin_stride),
                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_offset) & 0xFFFFFFFFFFFFFFFF, int(flags), schedule_ptr, offset_ptr,
                        ray_indices, int(rays_per_origin), target_columns, int(target_stride), *outs,
                        *((1, 0) if frames is None else (int(frames[0]), int(frames[1]))), int(adjoint_slots_per_item))
