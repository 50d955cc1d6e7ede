"""One target frame's optimisation loop: the hot path of scripts/main.py:323-865 assembled from the device pieces.

    detector() -> multi-view projection (HIP) -> Hungarian matching (HIP, on the device) -> projection losses
    -> schedules -> field block -> ray sampling -> fused two-pass render (HIP) -> silhouette (+ eikonal) loss
    -> backward (HIP adjoint kernels + torch for the tiny decode) -> Adam -> ExponentialLR

With ``graph=True`` the whole step is captured once per phase in a hipGraph (torch.cuda.CUDAGraph) and replayed: at 1000
rays the step is ~360 small launches and host-bound, and nothing in it needs the host any more -- the matching runs on the
device, and everything that changes from step to step (schedules, Philox counter, Adam step, learning rates) lives in
device memory that the kernels read (vsrd_render_config::device_schedule / device_stream_offset).

Frames are independent problems (README.md:128): multi-GPU runs shard *frames* over ranks (vsrd_amd/launcher.py) and
never exchange gradients.
"""
from dataclasses import InitVar, dataclass, field as dataclass_field
from typing import Optional, Sequence

import ctypes
import math
import threading
import time

import torch

from . import _lib, fields, frames, losses, models, operations, rendering


class _CaptureGate:
    """Stream capture against everything else, over the frames that one rank optimises concurrently (launcher.run_frames).  Capture is a
    process-wide mode, and every collision seen in round 4 -- each one a dead rank -- had a capture on one side: torch refuses a replay
    during another thread's capture ("Cannot prepare for replay during capturing stage": every graph registers the process-wide default
    generator); ROCm's ~CUDAGraph synchronises the device, which HIP refuses during a capture; HIP refuses, now and then, even a STREAM
    synchronisation (`.item()`, `.cpu()`, `stream.synchronize()`, `torch.nonzero`, a module's `.to(device)`) of one thread while another
    captures -- or lets it through and breaks the capture instead ("capturing stream has unjoined work"; a graph from such a capture is
    the likely cause of the one segmentation fault inside hipGraphLaunch).  So:
      ``with gate.capture():``  a capture -- alone: nothing else of any frame calls into HIP meanwhile (a waiting capture goes first);
      ``with gate:`` / ``acquire`` / ``release`` / ``with gate.replaying():``  everything else that calls into HIP from a frame's thread --
      construction, eager warm-up steps, replay launches, graph destruction, host synchronisations and copies: any number at once, never
      during a capture.  Nestable, also inside the capturing thread's own capture.
    ``acquire(blocking=False)``: the garbage collector's path; it never waits, and inside the capturing thread it is refused.
    (Two stricter gates came first: with EVERY call taking turns, replay launches included, the gain of several frames in flight was
    gone, 0.85 -> 0.75 frames/s -- a launch blocks for milliseconds behind the previous launch of the same graph; with only the launches
    shared, a frame still held the gate exclusively for 0.22-0.25 s of its 1.33 s.)"""

    def __init__(self):
        # (a re-entrant lock under the condition: the collector may run a FrameOptimizer's __del__ in a thread that is inside one of these
        #  few-line critical sections itself)
        self._state = threading.Condition(threading.RLock())
        self._capturer, self._capture_depth, self._waiting_captures, self._others = None, 0, 0, 0
        self._local = threading.local()
        self.capture_seconds, self._since = 0.0, 0.0            # total time spent capturing (launcher.main reports it per frame)

    def _depth(self):
        return getattr(self._local, "depth", 0)

    def acquire(self, blocking=True):
        me = threading.get_ident()
        with self._state:
            if self._capturer == me:
                if not blocking:             # the collector inside the capturing thread: not now
                    return False
                self._local.depth = self._depth() + 1           # (inside its own capture the capturing thread passes)
                return True
            if self._depth() > 0:            # nested: a capture that waits for THIS thread to leave must not stop it on the way out
                self._local.depth += 1
                return True
            while self._capturer is not None or self._waiting_captures:
                if not blocking:
                    return False
                self._state.wait()
            self._others += 1
            self._local.depth = 1
            return True

    def release(self):
        with self._state:
            self._local.depth -= 1
            if self._local.depth == 0 and self._capturer != threading.get_ident():
                self._others -= 1
                if not self._others:
                    self._state.notify_all()

    def __enter__(self):
        self.acquire()
        return self

    def __exit__(self, *exc):
        self.release()

    def replaying(self):
        return self

    def capture(self):
        return _CaptureTurn(self)


class _CaptureTurn:
    def __init__(self, gate):
        self.gate = gate

    def __enter__(self):
        gate, me = self.gate, threading.get_ident()
        with gate._state:
            if gate._capturer == me:
                gate._capture_depth += 1
                return
            if gate._depth() > 0:
                raise RuntimeError("a capture cannot start inside a section that holds the capture gate (it would wait for itself)")
            gate._waiting_captures += 1
            try:
                while gate._capturer is not None or gate._others:
                    gate._state.wait()
            finally:
                gate._waiting_captures -= 1
            gate._capturer, gate._capture_depth = me, 1
            gate._since = time.perf_counter()

    def __exit__(self, *exc):
        gate = self.gate
        with gate._state:
            gate._capture_depth -= 1
            if gate._capture_depth == 0:
                gate.capture_seconds += time.perf_counter() - gate._since
                gate._capturer = None
                gate._state.notify_all()


_capture_lock = _CaptureGate()


class _InitialDraw:
    """Seeding torch's host generator and drawing a frame's initial parameters from it: one frame at a time, and on ONE host thread -- the
    draw is a handful of tiny CPU operations (the largest: weight_norm over [1617, 256]), and on a 256-core box torch's intra-op pool takes
    100-200 ms to run them on all cores where one thread takes 2 ms (tools/reset_timers.py: a frame slot's reset() 100 ms -> 4.4 ms; the
    launcher lost 0.11 s per frame to it).  The values drawn do not depend on the thread count."""

    def __init__(self):
        self._lock = threading.Lock()

    def __enter__(self):
        self._lock.acquire()
        self._threads = torch.get_num_threads()
        if self._threads > 1:
            torch.set_num_threads(1)
        return self

    def __exit__(self, *exc):
        if self._threads > 1:
            torch.set_num_threads(self._threads)
        self._lock.release()


_initial_draw = _InitialDraw()


def exclusive_device_access():
    """``with exclusive_device_access(): ...`` -- no frame of this process captures meanwhile: for the host synchronisations and
    device-to-host copies (`.item()`, `stream.synchronize()`, checkpoints) of a frame that is optimised next to others."""
    return _capture_lock


_graveyard = []          # graphs whose owner went away while somebody captured: destroyed by the next holder of the lock


def _destroy_graphs(graphs, wait=True):
    """Destroy captured graphs where nobody captures.  On ROCm ``torch.cuda.CUDAGraph``'s destructor synchronises the DEVICE, which HIP
    refuses while any thread of the process is capturing ("operation not permitted when stream is capturing": the frames/s launcher
    lost a rank about once in five runs when one frame ended during the other frame's capture).  ``wait=False`` (garbage collection:
    the collector may run inside the capturing thread itself) parks the graphs instead of blocking."""
    if not graphs and not _graveyard:
        return
    if _capture_lock.acquire(blocking=wait):
        try:
            graphs.clear()
            _graveyard.clear()
        finally:
            _capture_lock.release()
    else:
        _graveyard.append(list(graphs.values()))
        graphs.clear()


class UnsuitableFrameError(ValueError):
    """A frame that cannot be served by a persistent frame slot (its importance weights do not suit the slot's table sampler)."""


@dataclass
class FrameInputs:
    """What scripts/main.py:106-316 prepares for one target frame; view 0 is the target view."""
    image_size: Sequence[int]               # (H, W)
    intrinsic_matrices: torch.Tensor        # [V,3,3]
    extrinsic_matrices: torch.Tensor        # [V,4,4] (target-camera frame -> view camera frame)
    soft_masks: torch.Tensor                # [V,H,W,N] re-indexed to the target's instance order (main.py:204-265)
    boxes_2d: torch.Tensor                  # [V,N,2,2] ground-truth 2-D boxes, zeros where invisible
    visible_masks: torch.Tensor             # [V,N] bool
    # 3-D ground truth for metrics() (main.py:877-886: target_inputs.boxes_3d and the dataset's rectification matrix), optional
    boxes_3d: Optional[torch.Tensor] = None              # [N,8,3] corners in the target's instance order, in the frame of the decoded boxes; NaN rows = no annotation
    rectification_matrix: Optional[torch.Tensor] = None  # [3,3] (None: identity)
    # the frame's group for group_labels() (make_predictions.py:50-60: the frames that get labels, the target among them), all five or none.
    # Keyword arguments and attributes like the fields above, but init-only: the dataclass's FIELDS stay what callers splat into it positionally
    # (dataclasses.fields ends with the 3-D ground truth; dataclasses.replace carries these over through their defaults)
    label_frame_ids: InitVar[Optional[torch.Tensor]] = None             # [L] int64
    label_intrinsic_matrices: InitVar[Optional[torch.Tensor]] = None    # [L,3,3]
    label_extrinsic_matrices: InitVar[Optional[torch.Tensor]] = None    # [L,4,4] (target-camera frame -> label view's camera frame)
    label_boxes_2d: InitVar[Optional[torch.Tensor]] = None              # [L,N,4] (xmin, ymin, xmax, ymax) in the target's instance order, zeros where invisible
    label_visible: InitVar[Optional[torch.Tensor]] = None               # [L,N] uint8 / bool
    # the views' colour images for the photometric term (main.py:689-853: target_inputs.images / source_inputs.images), init-only like the group
    images: InitVar[Optional[torch.Tensor]] = None                      # [V,3,H,W] float32 in 0..1

    def __post_init__(self, label_frame_ids, label_intrinsic_matrices, label_extrinsic_matrices, label_boxes_2d, label_visible, images=None):
        self.label_frame_ids, self.label_intrinsic_matrices, self.label_extrinsic_matrices = label_frame_ids, label_intrinsic_matrices, label_extrinsic_matrices
        self.label_boxes_2d, self.label_visible = label_boxes_2d, label_visible
        self.images = images


@dataclass
class OptimizationConfig:
    """configs/kitti_360/vsrd/*/config.json:120-127,166-238."""
    num_steps: int = 3000
    warmup_steps: int = 1000
    num_rays: int = 1000
    num_samples: int = 100
    distance_range: Sequence[float] = (0.0, 100.0)
    max_sdf_union_temperature: float = 1.0
    min_sdf_union_temperature: float = 0.1
    max_sdf_std_deviation: float = 1.0
    min_sdf_std_deviation: float = 0.1
    learning_rate: float = 1.0e-2
    embedding_learning_rate: float = 1.0e-3       # config.json:193-196
    hypernetwork_learning_rate: float = 1.0e-4    # config.json:197-200
    lr_gamma: float = 0.01 ** (1.0 / 3000.0)
    loss_weights: dict = dataclass_field(default_factory=lambda: dict(losses.LOSS_WEIGHTS))
    seed: int = 0
    skip_exact_misses: bool = True
    # the residual phase's per-instance MLP on split-bf16 matrix products (VSRD_FLAG_MLP_SPLIT_BF16; csrc/residual.h): the same tests within the
    # same tolerances as the exact-fp32 products (against the reference's goldens: labels within 1.1e-6 (tolerance 1e-4), gradients within 4.2e-4 of the largest entry (tolerance 5e-3; exact fp32: 1.5e-4)), the
    # residual step 8 % faster.  False: the exact-fp32 matrix instruction (the C ABI's own default).  The launcher's line names the form (`mlp_products`).
    mlp_split_bf16: bool = True
    # vsrd_render_config::adjoint_slots_per_item of the residual step (0: the library plans it from one frame's launch: 4 slots at 1000 rays).
    # A FrameBatch whose config leaves this at 0 picks the number for its B-fold item count (FrameBatch.item_slots: 16 for 8 x 1000 rays);
    # a frame walks bit-identical trajectories alone and in a batch when both use the same number.
    mlp_adjoint_item_slots: int = 0
    # The initial parameters (a detector's embeddings, the hypernetwork) are drawn from torch's global generator when a loop is built or reset.
    # None: whatever state that generator is in (the reference seeds it once per rank, scripts/main.py:67-74, so a frame's start depends on the
    # frames its rank optimised before).  An integer: the generator is seeded with it right before the draw -- a frame's result then depends on
    # the frame alone, not on the rank, process or slot that runs it (vsrd_amd.launcher passes seed and frame number).
    init_seed: Optional[int] = None
    # sphere tracing of the dense predicted masks (FrameOptimizer.masks; scripts/main.py:1029-1041 calls sphere_tracing with these)
    surface_num_iterations: int = 1000
    surface_convergence_criteria: float = 0.01
    surface_bounding_radius: float = 100.0
    # the photometric term (scripts/main.py:689-853; live when loss_weights["photometric_loss"] is non-zero, in the steps >= warmup_steps): the
    # rays drawn from the target view's hard masks per step and the patch of the correlation (config.json:216-225), the literal 4 of main.py:845;
    # its trace takes the three surface_* constants above
    surface_num_rays: int = 100
    surface_patch_size: Sequence[int] = (11, 11)
    surface_top_k: int = 4
    # the device-side log of the fused-glue graph loop (csrc/frame_log.h; scripts/main.py:870-953, 1109-1121 -- config.json's scalar_intervals
    # 50 and ckpt_intervals 500): every `scalar_interval` steps a row of scalars (FrameOptimizer.history), every `checkpoint_interval` steps a
    # snapshot of the models (FrameOptimizer.snapshots).  0: off -- no buffer, no launch, the loop as it is without them.
    scalar_interval: int = 0
    checkpoint_interval: int = 0

    def __post_init__(self):
        for name in ("scalar_interval", "checkpoint_interval"):
            if int(getattr(self, name)) < 0:
                raise ValueError(f"{name}: at least 0 (0: off), got {getattr(self, name)}")


LOG_LOSSES = ("iou_projection_loss", "l1_projection_loss", "silhouette_loss", "eikonal_loss", "loss")       # the epilogue's record, in order


def _align4(count):
    return (int(count) + 3) // 4 * 4


def _log_slot_layout(detector, hyper_distance_field, capacity):
    """[(name, tensor or None, floats reserved)] of a snapshot slot -- every entry starts on a multiple of four floats: the detector's four
    parameters laid out for `capacity` instances, every parameter of the hypernetwork, then the metrics summary [8] and the mask pixel counts
    [capacity,3] (int32), whose sources exist only once those outputs do.  Works on meta modules (sizes only)."""
    entries = [(f"detector.{name}", p, _align4(int(capacity) * p[0, 0].numel())) for name, p in detector.named_parameters()]
    entries += [(f"hyper_distance_field.{name}", p, _align4(p.numel())) for name, p in hyper_distance_field.named_parameters()]
    entries += [("summary", None, 8), ("counts", None, _align4(3 * int(capacity)))]
    if len(entries) > _lib.FRAME_LOG_SEGMENTS:
        raise ValueError(f"a snapshot of {len(entries)} tensors: vsrd_frame_log copies at most {_lib.FRAME_LOG_SEGMENTS} segments")
    return entries


def _steps_to_log_boundary(members):
    """Steps until the first of `members` reaches a boundary of either interval of the log (None: no log)."""
    cfg = members[0].config
    gaps = [interval - m.step_index % interval for m in members for interval in (cfg.scalar_interval, cfg.checkpoint_interval) if interval > 0]
    return min(gaps) if gaps and members[0]._log is not None else None


def _launch_log(members, frames=None):
    """After a step group of `members` (one loop, or the active rows of a batch whose row 0 leads the launches): when a member's step count
    sits on a boundary of the log, the metrics launch (every boundary) and the masks launch (checkpoint boundaries) whose buffers the log
    reads (a frame without ``boxes_3d`` gets the summary of no pair: count 0), then ONE vsrd_frame_log launch, all on the current stream -- the one the graphs replay on -- with no synchronisation.  Each row
    decides by its own device counter what it logs (csrc/frame_log.h), so a launch that a row did not need writes nothing in that row."""
    lead = members[0]
    log = lead._log
    if log is None:
        return
    cfg = lead.config
    due = [any(m.step_index > 0 and m.step_index % interval == 0 for m in members) if interval > 0 else False
           for interval in (cfg.scalar_interval, cfg.checkpoint_interval)]
    if not any(due):
        return
    started = time.perf_counter()
    if log["metrics"]:       # (always: a frame without boxes_3d has NaN ground truth in its row, so its summary comes out as count 0 -- never a
        lead._launch_output("metrics", frames=frames)        # summary an earlier frame of the row left behind)
    if log["masks"] and due[1]:
        lead._launch_output("masks", frames=frames, view=0)
    config = _lib.FrameLogConfig.from_buffer_copy(log["config"])
    config.num_frames, config.frame_stride = (1, 0) if frames is None else (int(frames[0]), int(frames[1]))
    with _capture_lock:
        _lib.check(_lib.load().vsrd_frame_log(config, _lib.stream()))
    lead.log_seconds += time.perf_counter() - started


def _steps_in_next_group(remaining, to_phase_end, to_log, steps_per_graph, one_step_graph_held):
    """How many steps the next graph launch of a ``run()`` takes: ``steps_per_graph`` or 1.  Whole groups only: a tail shorter than a group
    replays the one-step graph (every distinct k would otherwise cost a capture of its own -- a synchronisation -- for one use).  No group
    crosses the end of its phase (``to_phase_end``; None: the residual phase, which ends with the run) or a boundary of the log (``to_log``;
    None: no log -- the log's launch follows the group), and the phase's eager warm-up steps and its one-step graph come first."""
    k = int(steps_per_graph)
    room = min(bound for bound in (remaining, to_phase_end, to_log) if bound is not None)
    return k if k > 1 and one_step_graph_held and room >= k else 1


def _advance(owner, key, k, body, static=None):
    """THE capture/replay protocol of graph mode: ``k`` steps of ``owner`` (a FrameOptimizer, a FrameBatch) under ``key`` of its ``_graphs``.
    Three eager steps per one-step key on a side stream warm the allocator and the lazy initialisations -- they run the same device-side
    code, so they are ordinary optimisation steps -- then the step is captured once and replayed; a k-step graph is captured at its first
    use.  ``body(static, count=False, joins=...)`` launches one step and does not count it: the caller counts the k steps afterwards.
    ``static``: a tensor of the caller's that the body reads (explicit ray indices): an eager step reads it as it is, a capture reads a
    clone that the graph keeps, and every replay copies the caller's values into that clone first.  Returns the body's last result (of the
    capture, for a replay: device tensors that every replay rewrites)."""
    device = owner.device
    if key in owner._graphs:
        graph, kept, outputs = owner._graphs[key]
        with _capture_lock.replaying():      # (the copy too: nothing of a frame calls into HIP during another frame's capture)
            if kept is not None:
                kept.copy_(static)
            graph.replay()
        return outputs
    done = owner._eager_graph_steps.get(key, 0)
    if k == 1 and done < 3:
        with _capture_lock:          # (a phase's three eager steps too: nothing of a frame calls into HIP next to another frame's capture)
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):
                outputs = body(static, count=False, joins=(True, True))
            torch.cuda.current_stream(device).wait_stream(side)
        owner._eager_graph_steps[key] = done + 1
        return outputs
    kept = static.clone() if static is not None else None
    graph = torch.cuda.CUDAGraph()
    # an own capture stream per owner: torch keys the rocBLAS / hipBLASLt workspaces by stream, and its default capture stream is
    # shared by every capture -- two loops replayed at the same time would then run their GEMMs in one workspace
    if owner._capture_stream is None:
        owner._capture_stream = torch.cuda.Stream(device=device)
    # stream capture is a process-wide mode: one capture at a time, and thread-local error checking so that another frame's
    # thread (launcher.run_frames(frames_in_flight=2)) may keep replaying its own graph meanwhile
    # (no device-wide synchronisation out here: while ANOTHER frame's thread captures, HIP refuses it -- "operation not permitted when
    #  stream is capturing"; torch.cuda.graph synchronises by itself once this thread holds the lock and nobody captures)
    with _capture_lock.capture():
        with torch.cuda.graph(graph, stream=owner._capture_stream, capture_error_mode="thread_local"):
            for j in range(k):  # the hypernetwork's branch is joined to the step's stream only at the ends of the graph: between two
                # steps the next prologue (which needs the epilogue only) overlaps the hypernetwork's backward and forward
                outputs = body(kept, count=False, joins=(j == 0, j == k - 1))
        owner._graphs[key] = (graph, kept, outputs)
        # capture does not execute: this replay IS the step(s).  A graph's FIRST launch stays inside the capture's turn: next to another
        # thread's launch it died inside hipGraphLaunch (one 36-frame run in twelve; later launches of an uploaded graph have not)
        graph.replay()
    return outputs


def _capture_phases(members, k, step, group):
    """The walk of ``capture_all()`` over ``members`` (the loops that step together): in each phase ``step()`` four times -- three eager
    steps, then the capture (and first replay) of the one-step graph -- and ``group()``, the k-step group as ``run()`` takes it, where
    ``run()`` would (whole groups of k inside a phase, behind the one-step graph).
    (With the log these steps launch it too, with the metrics and masks launches in front of it, at counters that start from phase_start
    -- rows and slots of steps the founder never ran.  Harmless: the caller's reset() starts the log over, and every row a real run logs is
    written, metrics included, by that run's own launches.)"""
    cfg = members[0].config
    for phase_start in sorted({0, min(cfg.warmup_steps, cfg.num_steps)}):
        phase_steps = (cfg.warmup_steps if phase_start < cfg.warmup_steps else cfg.num_steps) - phase_start
        if phase_steps <= 0:
            continue
        with _capture_lock:
            for m in members:
                m.step_index = phase_start
                m.step_tensor.fill_(phase_start)
        for _ in range(min(4, phase_steps)):
            step()
        if k > 1 and phase_steps >= 4 + k:
            group()


class FrameArena:
    """Device memory of a BATCH of frames (include/vsrd_hip.h, "frame batches"): one row of ``row_bytes`` per frame, and every buffer a
    frame's kernels touch sits at the SAME offset of its frame's row -- frame f's copy of a buffer is ``stride`` bytes x f behind frame 0's,
    which is all a batched launch needs to know.  The rows are filled by the frames' own constructors (``FrameRow.new``): same calls in the
    same order give the same offsets, which ``FrameBatch`` verifies."""

    ALIGNMENT = 256

    @staticmethod
    def aligned(nbytes):
        """`nbytes` rounded up to where the next buffer of a row starts: the ONE alignment rule of rows, strides and FrameBatch._row_bytes."""
        return (int(nbytes) + FrameArena.ALIGNMENT - 1) // FrameArena.ALIGNMENT * FrameArena.ALIGNMENT

    def __init__(self, num_frames, row_bytes, device):
        self.stride = self.aligned(row_bytes)
        self.buffer = torch.empty(int(num_frames), self.stride, dtype=torch.uint8, device=device)
        self.rows = [FrameRow(self, f) for f in range(int(num_frames))]


def _buffer_bytes(shape, dtype):
    return math.prod(int(x) for x in shape) * torch.empty((), dtype=dtype).element_size()


class FrameRow:
    """Bump allocator over one frame's row of a ``FrameArena``."""

    def __init__(self, arena, index):
        self.arena, self.index = arena, index
        self.cursor = 0
        self.layout = []                 # (offset, nbytes) of every buffer, in order: equal across the rows of an arena

    def bytes(self, nbytes):
        nbytes = int(nbytes)
        offset = self.cursor
        end = offset + nbytes
        if end > self.arena.stride:
            raise RuntimeError(f"frame arena row of {self.arena.stride} bytes exhausted ({end} needed): FrameBatch._row_bytes is too small")
        self.cursor = FrameArena.aligned(end)
        self.layout.append((offset, nbytes))
        return self.arena.buffer[self.index, offset:end]

    def new(self, shape, dtype=torch.float32, fill=None):
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        view = self.bytes(_buffer_bytes(shape, dtype)).view(dtype).view(shape)
        if fill is not None:
            view.fill_(fill)
        return view

    def adopt(self, tensor):
        """A row-resident copy of `tensor` (same shape, dtype and values)."""
        return _place(tensor, tensor.shape, tensor.dtype, self)


def _instance_prefix(tensor, count):
    """The first `count` instances of a [1, capacity, ...] buffer of a mixed batch's row, as a contiguous [1, count, ...] view."""
    return tensor.as_strided((tensor.shape[0], int(count), *tensor.shape[2:]), tensor.stride(), tensor.storage_offset())


def _place(tensor, shape, dtype, row=None, private=False):
    """The ONE rule for where a loop's buffer lives: `tensor` as a `dtype` buffer of the FULL `shape` (views along dimension 0, instances
    behind them: the kernels stride by the capacities), the tensor in its leading corner and zeros around it.  `row` (a FrameRow): the
    buffer lies in the row.  No row, `private` (a frame slot): a buffer of its own -- a slot OWNS what reset() overwrites; float32
    contiguous inputs would otherwise be these very tensors: the caller's, and every other slot's built from the same frame.  Neither:
    the tensor ITSELF where it already has the shape, dtype and contiguity (a loop of one frame aliases the caller's soft masks --
    V x 376 x 1408 x N floats at the reference's size), a converted copy otherwise."""
    shape = tuple(int(x) for x in shape)
    if row is None and not private:
        if tuple(tensor.shape) != shape:
            raise ValueError(f"a buffer of shape {shape} cannot alias a tensor of shape {tuple(tensor.shape)}")
        return tensor.to(dtype).contiguous()
    full = row.new(shape, dtype, fill=0) if row is not None else torch.zeros(shape, dtype=dtype, device=tensor.device)
    corner = full
    for dim, size in enumerate(tensor.shape):
        corner = corner.narrow(dim, 0, size)
    corner.copy_(tensor)
    return full


def _incoming_shape(inputs, shape, capacities=None):
    """(V, H, W, N) of the frame -- a frames.FramePack or a FrameInputs -- that a loop of `shape` = (V, H, W, N) is asked to take over
    (FrameOptimizer.reset), or ValueError: the image size is the loop's; the counts are the loop's own, or with `capacities` =
    (view capacity, instance capacity) -- a row with a header -- anything from 1 up to them."""
    if isinstance(inputs, frames.FramePack):
        # (a pack counts its instances in its target view: without views it has none)
        incoming = (int(inputs.num_views), *[int(x) for x in inputs.image_size], int(inputs.num_instances) if inputs.num_views else 0)
    else:
        incoming = tuple(int(x) for x in inputs.soft_masks.shape)
        if tuple(int(x) for x in inputs.image_size) != incoming[1:3]:
            raise ValueError(f"image_size {tuple(inputs.image_size)} of soft masks of shape {incoming}")
    shape = tuple(int(x) for x in shape)
    if incoming[1:3] != shape[1:3]:
        raise ValueError(f"this loop serves frames of image size {shape[1:3]}, got {incoming[1:3]}")
    for k, (axis, name) in enumerate(((0, "views"), (3, "instances"))):
        low, high = (shape[axis], shape[axis]) if capacities is None else (1, int(capacities[k]))
        if not low <= incoming[axis] <= high:
            raise ValueError(f"this loop serves frames of {low}..{high} {name}, got {incoming[axis]}")
    return incoming


def _check_ground_truth(inputs, num_instances):
    """ValueError unless the optional 3-D ground truth of `inputs` -- a frames.FramePack or a FrameInputs -- has the shapes [N,8,3] and [3,3]:
    checked before a loop writes anything of the frame (construction of the metric buffers, FrameOptimizer.reset)."""
    for name, shape in (("boxes_3d", (int(num_instances), 8, 3)), ("rectification_matrix", (3, 3))):
        value = getattr(inputs, name, None)
        if value is not None and tuple(int(x) for x in value.shape) != shape:
            raise ValueError(f"{name} of shape {tuple(value.shape)} for a frame of {int(num_instances)} instances: expected {shape}")


def _initial_rates(config):
    """The initial learning rates of the optimiser's five groups (locations, dimensions, orientations, embeddings, hypernetwork)."""
    return [config.learning_rate] * 3 + [config.embedding_learning_rate, config.hypernetwork_learning_rate]


def _fresh_modules(num_instances):
    """A frame's modules as scripts/main.py:106-199 builds them per frame: the detector and (config.json:143-156) the per-instance residual
    MLP 48->16->16->16->16->1 generated from 256-d embeddings.  Draws from torch's host generator (unless built on the meta device)."""
    return models.BoxParameters3D(1, num_instances), models.HyperDistanceField(48, [16, 16, 16, 16], 256, [256, 256, 256, 256])


def _indexed(device):
    """`device` with its index spelled out (the scratch buffers are keyed by device: one spelling of it)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def adam_state_tensors(optimizer, parameter, group, row=None, capacity=None):
    """`parameter`'s torch.optim.Adam(capturable=True) state as the C ABI's pointer block, created now if the optimiser has not
    stepped yet (torch creates it lazily): the kernels update the moments, the counter and the parameter in place.  `row`: the frame's
    row of a batch's arena (FrameRow) -- the state is created there.  `capacity`: the parameter is [1, N, ...] and its moments are the
    first N instances of [1, capacity, ...] buffers (every row of a FrameBatch: FrameOptimizer.rebind passes the loop's capacity, which is N
    itself unless the batch has max_instances -- the same bytes at the same addresses as buffers of the parameter's own shape)."""
    state = optimizer.state[parameter]
    if not state:
        if row is not None:
            state["step"] = row.new((), torch.float32, fill=0.0)
            shape = parameter.shape if capacity is None else (parameter.shape[0], int(capacity), *parameter.shape[2:])
            state["exp_avg"], state["exp_avg_sq"] = row.new(shape, torch.float32, fill=0.0), row.new(shape, torch.float32, fill=0.0)
            if capacity is not None:
                state["exp_avg"] = _instance_prefix(state["exp_avg"], parameter.shape[1])
                state["exp_avg_sq"] = _instance_prefix(state["exp_avg_sq"], parameter.shape[1])
        else:
            state["step"] = torch.zeros((), dtype=torch.float32, device=parameter.device)
            state["exp_avg"], state["exp_avg_sq"] = torch.zeros_like(parameter), torch.zeros_like(parameter)
    return _lib.AdamTensors(parameter.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), state["step"].data_ptr(),
                            group["lr"].data_ptr())


def hypernetwork_tensors(hyper_distance_field, embeddings, optimizer, lr_gamma, row=None, capacity=None):
    """include/vsrd_hip.h::vsrd_hypernetwork over the torch module's own parameters and the optimiser's own state.  `optimizer`'s
    groups: the one holding `embeddings` and the one holding the hypernetwork, learning rates as device tensors."""
    def group_of(p):
        return next(g for g in optimizer.param_groups if any(q is p for q in g["params"]))
    net = _lib.Hypernetwork()
    net.num_instances, net.num_outputs = int(embeddings.shape[-2] if capacity is None else capacity), _lib.MLP_WEIGHTS
    betas = group_of(embeddings)["betas"]
    net.beta1, net.beta2, net.adam_epsilon, net.lr_gamma = float(betas[0]), float(betas[1]), float(group_of(embeddings)["eps"]), float(lr_gamma)
    net.embeddings = adam_state_tensors(optimizer, embeddings, group_of(embeddings), row, capacity)
    blocks = list(hyper_distance_field.hypernetwork)
    if len(blocks) != _lib.HYPER_LAYERS or embeddings.shape[-1] != 256 or not all(p.is_contiguous() for p in hyper_distance_field.parameters()):
        raise ValueError("csrc/hypernetwork.h is built for config.json:143-156: 256-d embeddings, four hidden blocks of 256")
    for l, block in enumerate(blocks):
        linear = block[0]
        net.weight_v[l], net.weight_g[l], net.bias[l] = (adam_state_tensors(optimizer, p, group_of(p), row) for p in (linear.weight_v, linear.weight_g, linear.bias))
        if l + 1 < len(blocks):
            net.norm_weight[l] = adam_state_tensors(optimizer, block[1].weight, group_of(block[1].weight), row)
            net.norm_bias[l] = adam_state_tensors(optimizer, block[1].bias, group_of(block[1].bias), row)
    return net


def mask_iou(counts):
    """inter / (pred + target - inter) of counts [...,3] = (#pred, #target, #pred and target), 0 where the union is empty."""
    counts = torch.as_tensor(counts)
    inter = counts[..., 2].to(torch.float32)
    union = (counts[..., 0] + counts[..., 1] - counts[..., 2]).to(torch.float32)
    return torch.where(union > 0, inter / union.clamp(min=1.0), torch.zeros_like(union))


# ---- what a frame can be asked for after its steps: labels(), masks(), metrics(), group_labels(), surface() ----------------------------
@dataclass(frozen=True)
class _FrameOutput:
    """What differs between the outputs; `FrameOptimizer._output_state` / `_launch_output` / `_ask` and `FrameBatch._ask` are the ONE path all take."""
    buffers: object                  # (V, N, H, W), the capacities -> [(name, shape, dtype, fill)] of what vsrd writes, in order: a plain function, no device
    launch: object                   # (loop, state, frame, header, **arguments) -> the status of the ONE vsrd_frame_* call; `frame`: the call's own frame config
    views: object                    # (loop, state, **arguments) -> the caller's dictionary: the buffers sliced to the frame's own V views / n instances
    last_step: Optional[str] = None  # what the output reads of the LAST STEP in the fused glue's tensors (it needs the glue AND a step to have run: the two needs coincide in today's outputs, one that had only one of them would split this field)
    leading: str = "view_capacity"   # the loop's capacity that is `V`, the buffers' leading dimension: "view_capacity" or "label_view_capacity"
    held: object = lambda switches: True             # (switches) -> whether a batch's row holds the buffers; `switches`: the keywords of FrameBatch._row_bytes, by name
    # an output that keeps INPUTS in its state has hooks for them, all run inside the capture gate under no_grad but `check`:
    check: object = lambda loop, inputs, n: None     # (loop, inputs, n): ValueError unless the frame `inputs` of n instances suits -- before anything is created, and by reset() before anything is overwritten
    write: object = lambda loop, state, n: None      # (loop, state, n): what the state keeps of the frame `loop.inputs` -- at creation and by every reset()
    take: object = lambda loop, state, **inputs: None        # (loop, state, **inputs): what the state keeps of ONE CALL's own inputs -- once per call, before its launch


def _check_asked(name, members):
    """RuntimeError unless the loops `members` -- one loop, or the active frames of a batch -- can be asked for output `name` now."""
    reads = _OUTPUTS[name].last_step
    if reads and not members[0].fused_glue:
        raise RuntimeError(f"{name}() reads the {reads} the fused glue keeps on the device (graph=True)")
    if reads and any(m.step_index < 1 or m.step_index != members[0].step_index for m in members):
        raise RuntimeError(f"{name}() reads the {reads} of the last step: no step has run since the loop was built or reset() (or, in a "
                           "batch, the frames are not in step)")


def _check_view(view, members, alone=False):
    """ValueError unless every one of the loops `members` has view `view`; `alone`: one loop's wording, which names its views."""
    if any(not 0 <= int(view) < m.num_views for m in members):
        raise ValueError(f"view: 0..{members[0].num_views - 1}, got {view}" if alone else f"view {view} does not exist in every active frame")


def _last_step_field(loop, asked):
    """(residual, field): whether the LAST STEP was a residual one, and the field it rendered -- the loop's instance block and, in the residual
    phase, its (centred) MLP weights -- for `asked`, the public method that renders it again: RuntimeError where a residual step left no weights."""
    residual = loop.step_index - 1 >= loop.config.warmup_steps
    if residual and not loop.fused_hypernetwork:
        raise RuntimeError(f"{asked}() in the residual phase reads the MLP weights csrc/hypernetwork.h leaves on the device")
    b = loop._glue
    return residual, _lib.make_field(b["instances"], 1.0, b["mlp_centred"] if residual else None)      # (the temperature comes from the device schedule)


def _write_label_tables(loop, state, n):
    """A loop without the fused glue has no tables on the device: float32 copies of its inputs' tables, kept in the state."""
    if not loop.fused_glue:
        state["tables"] = loop._input_tables()


def _label_buffers(V, N, H, W):
    f32 = torch.float32
    return [("camera_corners", (V, N, 8, 3), f32, 0.0), ("boxes_2d", (V, N, 4), f32, 0.0), ("mean_iou", (N, N), f32, 0.0),
            ("matched_gt", (N,), torch.int64, 0), ("confidences", (N,), f32, 0.0)]


def _launch_labels(loop, state, frame, header):
    # (a loop without the fused glue keeps float32 copies of its inputs' tables in the state: _write_label_tables)
    det, t = loop.detector, loop._glue if loop.fused_glue else state["tables"]
    return _lib.load().vsrd_frame_labels(
        frame, _lib.ptr(det.locations.data), _lib.ptr(det.dimensions.data), _lib.ptr(det.orientations.data), _lib.ptr(t["extrinsics"]),
        _lib.ptr(t["intrinsics"]), _lib.ptr(t["gt_boxes"]), t["visible"].data_ptr(), _lib.ptr(state["camera_corners"]), _lib.ptr(state["boxes_2d"]),
        _lib.ptr(state["mean_iou"]), state["matched_gt"].data_ptr(), _lib.ptr(state["confidences"]), header, _lib.stream())


def _label_views(loop, state):
    n, v = loop.num_instances, loop.num_views
    return dict(boxes_3d=state["camera_corners"][:v, :n], boxes_2d=state["boxes_2d"][:v, :n].unflatten(-1, (2, 2)), confidences=state["confidences"][:n],
                matched_gt=state["matched_gt"][:n], mean_iou=state["mean_iou"][:n, :n])


def _mask_buffers(V, N, H, W):           # (the bit-packed masks, the soft values and the pixel counts)
    return [("inside", (N, H, (W + 7) // 8), torch.uint8, 0), ("soft", (H * W, N), torch.float32, 0.0), ("counts", (N, 3), torch.int32, 0)]


def _launch_masks(loop, state, frame, header, view=0, threshold=0.5, soft=False):
    cfg, b = loop.config, loop._glue
    H, W = (int(x) for x in loop.inputs.image_size)
    from .rendering import renderers
    residual, field = _last_step_field(loop, "masks")
    flags = renderers._base_flags() & ~_lib.FLAG_MLP_SPLIT_BF16      # (exact-fp32 products)
    if residual:
        flags |= _lib.FLAG_MLP_WEIGHTS_CENTRED
    elif cfg.skip_exact_misses:
        flags |= _lib.FLAG_SKIP_EXACT_MISSES
    config = _lib.make_config(0, cfg.num_samples, cfg.distance_range, 1.0, 1.0, 1.0e-6, 3, seed=cfg.seed, stream_offset=loop.step_tensor, flags=flags,
                              schedule=loop.schedule, frames=(frame.num_frames, frame.frame_stride))
    masks = _lib.FrameMasksConfig(int(view), loop.view_capacity, H, W, int(cfg.surface_num_iterations), float(cfg.surface_convergence_criteria),
                                  float(cfg.surface_bounding_radius), float(threshold), loop.capacity)
    return _lib.load().vsrd_frame_masks(
        field, config, masks, _lib.ptr(loop.camera_positions), _lib.ptr(loop.ray_directions), None, None, _lib.ptr(b["masks"]),
        b["target_columns"].data_ptr(), state["inside"].data_ptr(), _lib.ptr(state["soft"]) if soft else None, state["counts"].data_ptr(),
        header, _lib.stream())


def _mask_views(loop, state, view=0, threshold=0.5, soft=False):
    n = loop.num_instances
    H, W = (int(x) for x in loop.inputs.image_size)
    counts = state["counts"][:n]
    result = dict(inside=state["inside"][:n], counts=counts, mask_iou=mask_iou(counts), threshold=float(threshold), shape=(H, W))
    if soft:
        result["soft"] = state["soft"].view(H, W, loop.capacity)[:, :, :n]
    return result


def _metric_buffers(V, N, H, W):
    """Beyond the glue's tensors: the ground-truth corners and the rectification matrix (read); the decoded corners, the IoUs, the summary."""
    f32, nan = torch.float32, float("nan")
    return [("gt_boxes_3d", (N, 8, 3), f32, nan), ("rectification", (3, 3), f32, 0.0), ("corners", (N, 8, 3), f32, 0.0), ("ious", (N, 2), f32, nan),
            ("summary", (8,), f32, 0.0)]


def _write_ground_truth(loop, state, n):
    """The row's ground-truth corners and rectification matrix from `loop.inputs`: NaN (no annotation) in every slot the frame does not
    fill -- all of them when the frame has no boxes_3d -- and the identity without a rectification matrix."""
    inp = loop.inputs
    state["gt_boxes_3d"].fill_(float("nan"))
    if inp.boxes_3d is not None:
        state["gt_boxes_3d"][:int(n)].copy_(inp.boxes_3d)
    state["rectification"].copy_(torch.eye(3) if inp.rectification_matrix is None else inp.rectification_matrix)


def _launch_metrics(loop, state, frame, header):
    det, b = loop.detector, loop._glue
    return _lib.load().vsrd_frame_metrics(
        frame, _lib.ptr(det.locations.data), _lib.ptr(det.dimensions.data), _lib.ptr(det.orientations.data), _lib.ptr(state["gt_boxes_3d"]),
        _lib.ptr(state["rectification"]), b["pd_indices"].data_ptr(), b["gt_indices"].data_ptr(), _lib.ptr(state["corners"]),
        _lib.ptr(state["ious"]), _lib.ptr(state["summary"]), header, _lib.stream())


def _metric_views(loop, state):
    n = loop.num_instances
    return dict(iou_3d=state["ious"][:n, 0], iou_bev=state["ious"][:n, 1], summary=state["summary"], corners=state["corners"][:n])


def label_view_count(inputs):
    """L of a frame -- a frames.FramePack or a FrameInputs: the label views of its group, 0 when it has none."""
    if isinstance(inputs, frames.FramePack):
        return int(inputs.num_label_views)
    ids = getattr(inputs, "label_frame_ids", None)
    return 0 if ids is None else int(ids.shape[0])


def _check_group(inputs, num_instances, capacity):
    """ValueError unless the optional group of `inputs` has the shapes of its L and the frame's N, and L fits a row laid out for `capacity`
    label views (0: the loop keeps no group, whatever the frame has): checked before a loop writes anything of the frame."""
    count = label_view_count(inputs)
    if count == 0 or capacity == 0:
        return
    if count > capacity:
        raise ValueError(f"a frame with {count} label views in a loop laid out for {capacity} (max_label_views)")
    shapes = dict(label_intrinsic_matrices=(count, 3, 3), label_extrinsic_matrices=(count, 4, 4), label_boxes_2d=(count, int(num_instances), 4),
                  label_visible=(count, int(num_instances)))
    for name, shape in shapes.items():
        value = getattr(inputs, name, None)
        if value is None or tuple(int(x) for x in value.shape) != shape:
            raise ValueError(f"{name} of shape {None if value is None else tuple(value.shape)} for a group of {count} views and {int(num_instances)} "
                             f"instances: expected {shape}")


def _write_group(loop, state, n):
    """The row's label-view tables and count from `loop.inputs`; a frame without a group leaves the count at 1 (group_labels() refuses it)."""
    inp = loop.inputs
    count = label_view_count(inp)
    state["count"].fill_(max(count, 1))
    state["frame_ids"].fill_(-1)
    if count:
        n = int(n)
        state["frame_ids"][:count].copy_(inp.label_frame_ids)
        state["extrinsics"][:count].copy_(inp.label_extrinsic_matrices.reshape(count, 16))
        state["intrinsics"][:count].copy_(inp.label_intrinsic_matrices.reshape(count, 9))
        state["gt_boxes"][:count, :n].copy_(inp.label_boxes_2d.reshape(count, n, 4))
        state["visible"][:count, :n].copy_(inp.label_visible.reshape(count, n))


def _group_buffers(L, N, H, W):
    """`L`: the label-view capacity.  The group's tables and the frame's own count (read), then vsrd_frame_group_labels' five outputs."""
    f32 = torch.float32
    return [("count", (1,), torch.int32, 1), ("frame_ids", (L,), torch.int64, -1), ("extrinsics", (L, 16), f32, 0.0), ("intrinsics", (L, 9), f32, 0.0),
            ("gt_boxes", (L, N, 4), f32, 0.0), ("visible", (L, N), torch.uint8, 0), ("camera_corners", (L, N, 8, 3), f32, 0.0),
            ("boxes_2d", (L, N, 4), f32, 0.0), ("mean_iou", (N, N), f32, 0.0), ("matched_gt", (N,), torch.int64, 0), ("confidences", (N,), f32, 0.0)]


def _launch_group_labels(loop, state, frame, header):
    det = loop.detector
    return _lib.load().vsrd_frame_group_labels(
        frame, _lib.ptr(det.locations.data), _lib.ptr(det.dimensions.data), _lib.ptr(det.orientations.data), loop.label_view_capacity,
        state["count"].data_ptr(), _lib.ptr(state["extrinsics"]), _lib.ptr(state["intrinsics"]), _lib.ptr(state["gt_boxes"]), state["visible"].data_ptr(),
        _lib.ptr(state["camera_corners"]), _lib.ptr(state["boxes_2d"]), _lib.ptr(state["mean_iou"]), state["matched_gt"].data_ptr(),
        _lib.ptr(state["confidences"]), header, _lib.stream())


def _group_views(loop, state):
    n, l = loop.num_instances, label_view_count(loop.inputs)
    return dict(boxes_3d=state["camera_corners"][:l, :n], boxes_2d=state["boxes_2d"][:l, :n].unflatten(-1, (2, 2)), confidences=state["confidences"][:n],
                matched_gt=state["matched_gt"][:n], mean_iou=state["mean_iou"][:n, :n], frame_ids=state["frame_ids"][:l])


def _surface_buffers(V, N, H, W):
    """What the caller hands over (the light, the instances' diffuse colours, the photograph), then vsrd_frame_surface's compact outputs.
    Positions and normals, the call's per-pixel float triples, are not kept (rendering.surface_render returns them)."""
    u8, f32 = torch.uint8, torch.float32
    return [("light", (3,), f32, 0.0), ("palette", (N, 3), f32, 0.0), ("background", (H * W, 3), u8, 0), ("converged_bits", (H, (W + 7) // 8), u8, 0),
            ("shadow_bits", (H, (W + 7) // 8), u8, 0), ("instance", (H * W,), u8, 255), ("range", (H * W,), f32, 0.0), ("colors", (H * W, 3), u8, 0)]


def _write_surface(loop, state, light=None, background=None):
    """The row's light, palette and photograph for the call's surface launch (host values: outside any capture)."""
    from .rendering import renderers
    H, W = (int(x) for x in loop.inputs.image_size)
    state["light"].copy_(torch.as_tensor(renderers.SURFACE_LIGHT if light is None else light, dtype=torch.float32).reshape(3))
    state["palette"].copy_(renderers.surface_palette(loop.capacity))
    if background is not None:
        if tuple(background.shape) != (H, W, 3) or background.dtype != torch.uint8:
            raise ValueError(f"background must be uint8 [H,W,3] = {(H, W, 3)}, got {background.dtype} {tuple(background.shape)}")
        state["background"].copy_(background.reshape(H * W, 3))


def _launch_surface(loop, state, frame, header, view=0, hard=True, shadows=True, background=False, alpha=None):
    cfg = loop.config
    H, W = (int(x) for x in loop.inputs.image_size)
    from .rendering import renderers
    _, field = _last_step_field(loop, "surface")
    config = _lib.make_config(0, cfg.num_samples, cfg.distance_range, 1.0, 1.0, 1.0e-6, 3, schedule=loop.schedule, frames=(frame.num_frames, frame.frame_stride))
    blend = (0.6 if background else 1.0) if alpha is None else float(alpha)
    surface = renderers.surface_config(view, loop.view_capacity, H, W, cfg.surface_num_iterations, cfg.surface_convergence_criteria,
                                       cfg.surface_bounding_radius, None, hard=hard, shadows=shadows, background=background, alpha=blend)
    return _lib.load().vsrd_frame_surface(
        field, config, surface, _lib.ptr(loop.camera_positions), _lib.ptr(loop.ray_directions), _lib.ptr(state["light"]), _lib.ptr(state["palette"]),
        state["background"].data_ptr() if background else None, state["converged_bits"].data_ptr(), state["shadow_bits"].data_ptr(),
        state["instance"].data_ptr(), _lib.ptr(state["range"]), state["colors"].data_ptr(), None, None, header, _lib.stream())


def _surface_views(loop, state, view=0, hard=True, shadows=True, background=False, alpha=None):
    H, W = (int(x) for x in loop.inputs.image_size)
    return dict(converged_bits=state["converged_bits"], shadow_bits=state["shadow_bits"], instance=state["instance"].view(H, W),
                range=state["range"].view(H, W), colors=state["colors"].view(H, W, 3), light=state["light"], shape=(H, W), view=int(view), hard=bool(hard))


# THE table of the outputs, in the order a row holds them.  group_labels: laid out for the LABEL-view capacity, in the rows of a batch that
# has one (max_label_views); surface: whole images per row (5.7 MB at 376 x 1408), in the rows of a batch built for it (surface=True)
_OUTPUTS = dict(
    labels=_FrameOutput(_label_buffers, _launch_labels, _label_views, write=_write_label_tables),             # csrc/frame_labels.h
    masks=_FrameOutput(_mask_buffers, _launch_masks, _mask_views, last_step="field block"),                   # csrc/frame_masks.h
    metrics=_FrameOutput(_metric_buffers, _launch_metrics, _metric_views, last_step="matching",               # csrc/frame_metrics.h
                         check=lambda loop, inputs, n: _check_ground_truth(inputs, n), write=_write_ground_truth),
    group_labels=_FrameOutput(_group_buffers, _launch_group_labels, _group_views, leading="label_view_capacity",          # csrc/frame_group_labels.h
                              held=lambda switches: switches["label_views"] > 0,
                              check=lambda loop, inputs, n: _check_group(inputs, n, loop.label_view_capacity), write=_write_group),
    surface=_FrameOutput(_surface_buffers, _launch_surface, _surface_views, last_step="field block",          # csrc/frame_surface.h
                         held=lambda switches: switches["surface"], take=_write_surface))


# ---- what a graph-mode loop keeps besides its outputs, declared as they are: plain functions of the capacities and the config ->
# [(name, shape, dtype, fill)] in the order of allocation, no device.  FrameOptimizer allocates from them (`_buffers`) and
# FrameBatch._row_bytes sums over them, so a buffer added to a family is in the size of a row
def _parameter_buffers(N):
    """The modules' parameters (the detector's laid out for N instances), then Adam's state of each as adam_state_tensors creates it."""
    with torch.device("meta"):               # (no memory, no random numbers drawn)
        named = [(f"{module}.{name}", tuple(p.shape)) for module, m in zip(("detector", "hyper_distance_field"), _fresh_modules(N))
                 for name, p in m.named_parameters()]
    f32 = torch.float32
    state = [[(f"{name}.step", (), f32, 0.0), (f"{name}.exp_avg", shape, f32, 0.0), (f"{name}.exp_avg_sq", shape, f32, 0.0)] for name, shape in named]
    return [(name, shape, f32, None) for name, shape in named] + sum(state, [])


def _scalar_buffers(config):
    """The learning rates of the optimiser's five groups and its default rate, the step counter (= Philox counter) and the schedule
    (temperature, std, cosine_ratio)."""
    rates = zip(("locations", "dimensions", "orientations", "embeddings", "hypernetwork", "default"), _initial_rates(config) + [config.learning_rate])
    return [(f"lr.{name}", (), torch.float32, value) for name, value in rates] + [("step_tensor", (1,), torch.int64, 0), ("schedule", (3,), torch.float32, 1.0)]


def _ray_buffers(V, N, H, W):
    """The rays of every view, the soft masks [V H W, N] (the kernels read the targets with target_stride = N) and the importance weights."""
    f32, pixels = torch.float32, V * H * W
    return [("camera_positions", (V, 3), f32, 0.0), ("ray_directions", (pixels, 3), f32, 0.0), ("flat_masks", (pixels, N), f32, 0.0),
            ("sampling_weights", (pixels,), f32, 0.0)]


def _table_buffers(V, N):
    """The frame's cameras, ground-truth boxes and visibility as the kernels read them."""
    f32 = torch.float32
    return [("extrinsics", (V, 16), f32, 0.0), ("intrinsics", (V, 9), f32, 0.0), ("gt_boxes", (V, N, 4), f32, 0.0), ("visible", (V, N), torch.uint8, 0)]


def _glue_buffers(V, N, config, headed):
    """The fused glue's (csrc/frame_step.h): the input tables, what the prologue, the render launch and the epilogue hand each other, with
    `headed` the row's vsrd_frame_header, and from `hyper_workspace` on what is created after the parameters' Adam state (rebind)."""
    lib, rays = _lib.load(), int(config.num_rays)
    f32, i32, i64, u8 = torch.float32, torch.int32, torch.int64, torch.uint8
    return _table_buffers(V, N) + [
        ("scratch", (lib.vsrd_frame_scratch_bytes(V, N),), u8, None), ("instances", (N, 16), f32, 0.0), ("pd_indices", (N,), i64, 0),
        ("gt_indices", (N,), i64, 0), ("target_columns", (N,), i32, 0), ("instance_weights", (N,), f32, 1.0), ("projection_losses", (2,), f32, 0.0),
        ("render_losses", (2,), f32, 0.0), ("grad_raw", (N, 8), f32, 0.0), ("raw_gradients", (N, 8), f32, 0.0), ("grad_instances", (N, 16), f32, 0.0),
        ("grad_mlp", (N, _lib.MLP_WEIGHTS), f32, 0.0), ("record", (5,), f32, 0.0)] + \
        ([("header", (ctypes.sizeof(_lib.FrameHeader),), u8, 0)] if headed else []) + [
        ("hyper_workspace", (lib.vsrd_hypernetwork_workspace_bytes(N),), u8, None), ("picks", (rays,), i64, 0), ("ray_indices", (rays,), i64, 0),
        ("mlp_weights", (N, _lib.MLP_WEIGHTS), f32, 0.0), ("mlp_centred", (N, _lib.MLP_WEIGHTS), f32, 0.0)]


def _log_capacity(N, config):
    """(history rows, snapshot slots, floats of a slot) of the log of a loop laid out for N instances."""
    rows = config.num_steps // config.scalar_interval if config.scalar_interval > 0 else 0
    slots = config.num_steps // config.checkpoint_interval if config.checkpoint_interval > 0 else 0
    with torch.device("meta"):
        layout = _log_slot_layout(*_fresh_modules(N), N)
    return rows, slots, sum(size for _, _, size in layout) if slots else 0


def _log_buffers(N, config):
    """The device-side log's (csrc/frame_log.h): history [rows, 22], snapshots [slots, slot], the slots' steps, the four counters, the list
    of the five rate pointers and the segment table."""
    rows, slots, slot_floats = _log_capacity(N, config)
    f32, i32 = torch.float32, torch.int32
    return [("history", (max(rows, 1), _lib.FRAME_LOG_COLUMNS), f32, 0.0), ("snapshots", (max(slots, 1), max(slot_floats, 4)), f32, 0.0),
            ("snapshot_steps", (max(slots, 1),), i32, -1), ("counters", (4,), i32, 0), ("rate_pointers", (5,), torch.int64, 0),
            ("table", (_lib.FRAME_LOG_SEGMENTS * ctypes.sizeof(_lib.LogSegment),), torch.uint8, 0)]


def photometric_weight(config):
    """The weight of the photometric term, 0.0 when it is off: the reference tests the weight's truthiness (scripts/main.py:689)."""
    return float(config.loss_weights.get("photometric_loss", 0.0) or 0.0)


def _photometric_buffers(V, N, H, W, config, fused=True):
    """The photometric term's (csrc/frame_photometric.h): the gray planes, the target view's hard-mask union as the weights of the term's
    draw, the drawn rays, and -- `fused`: the fused glue -- the workspace and the outputs of vsrd_frame_photometric.  (The ray table over
    the hard-mask weights, vsrd_ray_table_bytes(H W), follows them in graph mode.)"""
    f32, rays = torch.float32, int(config.surface_num_rays)
    pw, ph = (int(x) for x in config.surface_patch_size)
    declared = [("gray", (V, H, W), f32, 0.0), ("hard_weights", (H * W,), f32, 0.0), ("ray_indices", (rays,), torch.int64, 0)]
    if fused:
        declared += [("workspace", (_lib.load().vsrd_frame_photometric_workspace_bytes(N, 1, V, rays, pw * ph),), torch.uint8, None),
                     ("loss", (1,), f32, 0.0), ("stats", (2,), f32, 0.0), ("grad_instances", (N, 16), f32, 0.0),
                     ("grad_mlp", (N, _lib.MLP_WEIGHTS), f32, 0.0)]
    return declared


def _check_loss_weights(config):
    """ValueError for a loss weight the loops do not know: a term that nothing applies would otherwise be dropped without a word."""
    unknown = sorted(set(config.loss_weights) - set(losses.LOSS_WEIGHTS))
    if unknown:
        raise ValueError(f"loss_weights: unknown terms {unknown}; the loop applies {sorted(losses.LOSS_WEIGHTS)}")


def _check_photometric(inputs, config, num_views, num_instances):
    """ValueError unless a frame -- a frames.FramePack or a FrameInputs -- can be optimised with the photometric term of `config` (off: nothing
    is checked): its images, a silhouette weight to scale by, the limits of vsrd_frame_photometric and enough pixels in the target view's
    hard-mask union for a draw.  Needs no device: checked before a loop writes anything of the frame (construction, FrameOptimizer.reset)."""
    if photometric_weight(config) == 0.0:
        return
    if not float(config.loss_weights.get("silhouette_loss", 0.0) or 0.0):
        raise ValueError("the photometric term's gradients are accumulated in units of the silhouette term (csrc/frame_step.h): "
                         "loss_weights['silhouette_loss'] must not be 0")
    V, N, rays, k = int(num_views), int(num_instances), int(config.surface_num_rays), int(config.surface_top_k)
    patch = tuple(int(x) for x in config.surface_patch_size)
    if not 1 <= rays <= _lib.PHOTOMETRIC_RAYS:
        raise ValueError(f"surface_num_rays: 1..{_lib.PHOTOMETRIC_RAYS} (the table sampler's limit), got {rays}")
    if not 1 <= k <= V <= _lib.PATCH_VIEWS:
        raise ValueError(f"the photometric term needs 1 <= surface_top_k <= views <= {_lib.PATCH_VIEWS}, got top_k {k} and {V} views")
    if len(patch) != 2 or min(patch) < 1 or patch[0] * patch[1] > _lib.PATCH_PIXELS:
        raise ValueError(f"surface_patch_size: (width, height) of at most {_lib.PATCH_PIXELS} pixels, got {patch}")
    if not 1 <= N <= _lib.MAX_INSTANCES:
        raise ValueError(f"the photometric term serves 1..{_lib.MAX_INSTANCES} instances, got {N}")
    images = getattr(inputs, "images", None)
    if images is None:
        raise ValueError("loss_weights['photometric_loss'] is non-zero: the frame needs its images (FrameInputs.images [V,3,H,W]; a frame pack's "
                         "optional member `images`)")
    H, W = (int(x) for x in inputs.image_size)
    if tuple(int(x) for x in images.shape) != (V, 3, H, W):
        raise ValueError(f"images of shape {tuple(images.shape)} for a frame of {V} views of {H} x {W}: expected {(V, 3, H, W)}")
    if isinstance(inputs, frames.FramePack):
        return      # (a pack's soft masks exist on the device only: reset() counts the hard pixels once vsrd_frame_ingest has written them)
    hard = int((inputs.soft_masks[0].amax(dim=-1) > 0.5).sum())
    if hard < rays:
        raise ValueError(f"only {hard} pixels of the target view lie in a hard mask, fewer than surface_num_rays = {rays} "
                         "(torch.multinomial without replacement raises in the reference as well)")


class FrameOptimizer:
    """``graph=True``: the step is captured in a hipGraph and replayed.  ``fused_glue`` (default: on in graph mode): everything around
    the render launch that concerns the boxes -- decode, projection, matching, projection losses and their gradients, schedules,
    the chain rule through the decode, Adam and the learning-rate decay -- runs as two single-workgroup HIP kernels
    (csrc/frame_step.h) instead of ~330 torch element-wise launches, and the render kernel gathers its rays from the
    frame-resident tensors by index; in the residual phase the hypernetwork, its backward and its Adam are csrc/hypernetwork.h
    (``fused_hypernetwork = False`` keeps them with torch: the A/B reference)."""

    def __init__(self, inputs: FrameInputs, config: OptimizationConfig, device, graph=False, fused_glue=None, persistent=False, row=None,
                 capacity=None, view_capacity=None, max_label_views=None):
        """``persistent``: the loop will be given other frames of the same shape through ``reset()`` (a frame SLOT, launcher.py): it then
        owns every buffer a captured graph holds the address of -- in particular a copy of the soft masks instead of the caller's tensor.
        ``row`` (a ``FrameRow``): the loop is one frame of a ``FrameBatch`` and keeps EVERY device buffer its kernels touch -- parameters,
        Adam's state, rates, counters, rays, masks, sampling table, scratch -- in that row of the batch's arena.  ``capacity`` (with
        ``row``): the row of a MIXED batch (FrameBatch(max_instances=...)): every per-instance buffer is laid out for ``capacity``
        instances, the frame's own N fill the first rows, and the row's header (include/vsrd_hip.h, vsrd_frame_header) carries N.
        ``view_capacity`` (with ``row``; FrameBatch(max_views=...)): likewise every per-view buffer -- camera positions, ray directions,
        inverse projections, extrinsics and intrinsics, ground-truth boxes and visibility, soft masks, sampling weights, the ray table, the
        label outputs, the prologue's scratch -- is laid out for ``view_capacity`` views; they are view-major, so the frame's own V fill a
        prefix of each, and the header carries V and V H W.  Either capacity gives the row a header; the other one is then the founder's
        own count.
        ``max_label_views``: the label views (``FrameInputs.label_*``: the frame's group) that ``group_labels()`` lays its tables out for --
        None: the frame's own L; a loop that ``reset()`` gives other frames needs the largest L among them.  0: the loop keeps no group."""
        _check_loss_weights(config)
        _check_photometric(inputs, config, inputs.soft_masks.shape[0], inputs.soft_masks.shape[-1])
        self.label_view_capacity = label_view_count(inputs) if max_label_views is None else int(max_label_views)
        if not 0 <= self.label_view_capacity <= _lib.MAX_LABEL_VIEWS:
            raise ValueError(f"max_label_views: 0..{_lib.MAX_LABEL_VIEWS}, got {self.label_view_capacity}")
        if label_view_count(inputs) > self.label_view_capacity > 0:
            raise ValueError(f"a frame with {label_view_count(inputs)} label views in a loop laid out for {self.label_view_capacity} (max_label_views)")
        if config.scalar_interval > 0 or config.checkpoint_interval > 0:
            if not (graph and fused_glue in (None, True)):
                raise ValueError("scalar_interval / checkpoint_interval: the log is filled between the replays of the fused-glue graph loop "
                                 "(graph=True, fused_glue on); the eager loop has no device-side log")
        self._graphs = {}
        self.persistent = bool(persistent)
        self._row = row
        self._headed = capacity is not None or view_capacity is not None        # (a row with a header)
        if self._headed and row is None:
            raise ValueError("a capacity belongs to a frame of a FrameBatch (row=...)")
        if row is not None and not (graph and persistent and fused_glue in (None, True)):
            raise ValueError("a frame of a batch is a persistent graph-mode loop with the fused glue")
        # the whole construction stays out of other frames' captures: it copies modules to the device, reads ranges back (.item()), runs
        # nonzero -- host synchronisations that, next to ANOTHER frame's capture, fail now and then or break that capture ("capturing
        # stream has unjoined work" in the other thread: one 36-frame run in fourteen)
        with _capture_lock:
            self._construct(inputs, config, device, graph, fused_glue, capacity, view_capacity)

    def _construct(self, inputs, config, device, graph, fused_glue, capacity, view_capacity):
        self.inputs, self.config, self.device = inputs, config, _indexed(device)
        self.graph = bool(graph)
        self.fused_glue = self.graph if fused_glue is None else bool(fused_glue)
        if self.fused_glue and not self.graph:
            raise ValueError("fused_glue keeps the learning rates and Adam's counters on the device: it needs graph=True")
        V, H, W, N = inputs.soft_masks.shape
        self.num_views, self.num_instances = V, N
        # every loop lays its per-view and per-instance buffers out for (view_capacity, capacity): the frame's own counts unless the row has a header
        self.capacity = N if capacity is None else int(capacity)
        self.view_capacity = V if view_capacity is None else int(view_capacity)
        if not 1 <= N <= self.capacity:
            raise ValueError(f"a row of capacity {self.capacity} serves frames of 1..{self.capacity} instances, got {N}")
        if not 1 <= V <= self.view_capacity <= _lib.MAX_VIEWS:
            raise ValueError(f"a row of view capacity {self.view_capacity} (at most {_lib.MAX_VIEWS}) serves frames of 1..{self.view_capacity} views, got {V}")
        with _initial_draw:
            if config.init_seed is not None:
                torch.default_generator.manual_seed(int(config.init_seed))      # (the CPU generator: the modules are built on the host; the device generators, which captured graphs register, stay untouched)
            detector, field = _fresh_modules(N)
        self.detector, self.hyper_distance_field = detector.to(self.device), field.to(self.device)
        if self._row is not None:          # the parameters move into the frame's row (module order: the same in every frame of the batch)
            for p in self.detector.parameters():           # ([1, N, ...]: the first N instances of a buffer laid out for the capacity)
                p.data = _instance_prefix(self._place(p.data, (1, self.capacity, *p.shape[2:]), p.dtype), N)
            for p in self.hyper_distance_field.parameters():
                p.data = self._place(p.data, p.shape, p.dtype)
        # graph mode: learning rates are device tensors decayed in place inside the captured step
        scalars = _scalar_buffers(config)
        *rates, default = (self._buffers(scalars[:-2]) if self.graph else {name: value for name, _, _, value in scalars[:-2]}).values()
        groups = [dict(params=params, lr=lr) for params, lr in zip(self._module_parameters(), rates)]
        self.optimizer = torch.optim.Adam(groups, lr=default, capturable=self.graph)
        self.scheduler = None if self.graph else torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=config.lr_gamma)
        # per-step scalars on the device (graph mode): step index = Philox counter, (temperature, std, cosine_ratio)
        self.step_tensor, self.schedule = self._buffers(scalars[-2:]).values()
        # this frame's own scratch (frames may be optimised concurrently on other streams); freed with the optimizer.  Graph mode
        # sizes it for the residual phase up front: a captured graph holds the buffer's address
        self.workspace = rendering.Workspace(allocate=None if self._row is None else self._row.bytes)
        if self.graph:
            self.workspace.keep_outgrown = True          # a captured graph holds the buffer's address: an outgrown buffer must outlive it
            self.workspace.reserve(self.device, self.capacity, residual=True, step_shape=(config.num_samples, config.num_rays))
        self._graphs = {}
        self._outputs = {}                  # labels() / masks() / metrics(): the buffers of each, by name, created at its first use
        self._capture_stream = None
        self._eager_graph_steps = {}
        self.pixels_per_view = H * W
        self._prepare_rays(inputs, config, H, W, N)
        self.step_index = 0
        self._log, self.log_seconds = None, 0.0          # (the device-side log: _init_log)
        self._photometric = None                         # (the photometric term's buffers: _init_photometric)
        if self.fused_glue:
            self._init_fused_glue()
        if photometric_weight(config) != 0.0:
            self._init_photometric()

    def _new(self, shape, dtype=torch.float32, fill=None):
        """A device buffer of this loop: in the frame's row of the batch's arena when there is one."""
        if self._row is not None:
            return self._row.new(shape, dtype, fill)
        if fill is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return torch.full(shape if isinstance(shape, (tuple, list)) else (shape,), fill, dtype=dtype, device=self.device)

    def _place(self, tensor, shape, dtype=torch.float32):
        """`tensor` as this loop's buffer of the full `shape` (module-level `_place`): in the frame's row, a slot's own, or the tensor itself."""
        return _place(tensor.to(self.device), shape, dtype, self._row, self.persistent)

    def _buffers(self, declared, contents=None):
        """The buffers of a declaration -- [(name, shape, dtype, fill)]: _FrameOutput.buffers and the families above -- by name, created in
        its order by the one placement rule: the tensors of `contents` (by name) go into the leading corner of theirs (`_place`)."""
        contents = contents or {}
        return {name: self._place(contents[name], shape, dtype) if name in contents else self._new(shape, dtype, fill)
                for name, shape, dtype, fill in declared}

    def _input_tables(self):
        """The frame's cameras, ground-truth boxes and visibility as the kernels read them, laid out for the capacities."""
        inp, V, N = self.inputs, self.num_views, self.num_instances
        return self._buffers(_table_buffers(self.view_capacity, self.capacity),
                             dict(extrinsics=inp.extrinsic_matrices.reshape(V, 16), intrinsics=inp.intrinsic_matrices.reshape(V, 9),
                                  gt_boxes=inp.boxes_2d.reshape(V, N, 4), visible=inp.visible_masks))

    def _set_views(self, V):
        """The loop's per-view tensors are the first V views of its buffers (`self._full`: laid out for the view capacity) -- view-major,
        so contiguous prefixes at the buffers' own addresses, which is what the kernels and the captured graphs hold."""
        full, pixels = self._full, V * self.pixels_per_view
        self.num_views = V
        self.camera_positions, self.ray_directions = full["camera_positions"][:V], full["ray_directions"][:pixels]
        self.flat_masks, self.sampling_weights = full["flat_masks"][:pixels], full["sampling_weights"][:pixels]
        if "extrinsics" in full:              # (the glue's tables, once _init_fused_glue has made them)
            b = self._glue
            for name in ("extrinsics", "intrinsics", "gt_boxes", "visible"):
                b[name] = full[name][:V]
            b["masks"] = self.flat_masks

    def _write_header(self):
        """A mixed batch's row: the frame's own instance count and silhouette normaliser (the float32 the one-frame path passes by value),
        its own view count and the count of its sampling table (include/vsrd_hip.h, vsrd_frame_header: ABI 12)."""
        header = _lib.FrameHeader(self.num_instances | _lib.FRAME_HEADER_HAS_VIEWS, 1.0 / (self.config.num_rays * self.num_instances),
                                  self.num_views, 0, self.num_views * self.pixels_per_view)
        self._glue["header"].copy_(torch.frombuffer(bytearray(bytes(header)), dtype=torch.uint8))

    def _prepare_rays(self, inputs, config, H, W, N):
        # rays of every view, once per frame (main.py:267-296)
        cam, dirs = rendering.ray_casting((H, W), inputs.intrinsic_matrices, inputs.extrinsic_matrices)
        # [view capacity x H W, instance capacity] soft masks (the kernels read the targets with target_stride = capacity) and every other
        # per-view buffer laid out for the view capacity; the frame fills their leading corners.  (A slot's graphs read the masks through
        # this address for every later frame; a loop of one frame reads the caller's own tensor.)
        self._full = self._buffers(_ray_buffers(self.view_capacity, self.capacity, H, W),
                                   dict(camera_positions=cam, ray_directions=dirs.reshape(-1, 3), flat_masks=inputs.soft_masks.reshape(-1, N)))
        self._set_views(self.num_views)
        torch.amax(self.flat_masks[:, :N], dim=-1, out=self.sampling_weights)                                             # main.py:620-624
        self.ray_table = self.ray_remap = None
        if not self._prepare_sampler(config):
            raise UnsuitableFrameError("this frame's importance weights do not suit the table sampler (too much of the weight in fewer pixels "
                                       "than a draw needs; rendering.RayTable.suits): it cannot found a frame slot -- optimise it in a loop of "
                                       "its own (persistent=False), which keeps the per-step race sampler")

    def _prepare_sampler(self, config):
        """What depends on the frame's importance weights (fixed for the frame).  Graph mode draws the rays on the device: the sampler's
        table is built here, once per frame, over ALL V*H*W weights -- entries without weight have zero width and are never drawn, and the
        table's size and entry count depend on the frame's SHAPE only, so a slot's graphs (which hold the table's address and count) serve
        every frame of that shape; a step's draw is one launch (csrc/ray_sampling.h).  Frames whose weight sits in fewer entries than a
        draw needs keep the per-step exponential race over the positive pixels (`ray_table` None).  False: such a frame cannot take over a
        slot whose graphs were captured with the table."""
        positive = int((self.sampling_weights > 0).sum())
        # torch.multinomial(replacement=False) raises when fewer categories than samples have weight; the device sampler would pad
        # its output with -1 instead (ray_sampling.h), silently: the weights are fixed for the frame, so check once here
        if positive < config.num_rays:
            raise ValueError(f"only {positive} pixels have a positive soft mask, fewer than num_rays = {config.num_rays} "
                             "(torch.multinomial without replacement raises in the reference as well)")
        if not (self.graph and self.device.type == "cuda"):
            return True
        had_table = self.ray_table is not None
        if had_table:
            self.ray_table.rebuild(self.sampling_weights)
        # (a row laid out for a view capacity: the table's allocation is sized for capacity x H W weights, the table in it is the frame's own)
        table = self.ray_table if had_table else rendering.RayTable(self.sampling_weights, allocate=None if self._row is None else self._row.bytes,
                                                                    capacity=self.view_capacity * self.pixels_per_view)
        if table.suits(config.num_rays):
            self.ray_table = table
            return True
        if had_table or self.persistent:
            # a slot's graphs are captured with ONE sampler: a frame that does not suit the table cannot take over a slot (nor found one:
            # __init__ raises UnsuitableFrameError) -- the caller optimises it in a loop of its own, with the race sampler
            return False
        # the race sampler only visits the pixels that can be drawn at all
        self.positive_pixels = torch.nonzero(self.sampling_weights > 0).flatten()
        self.positive_weights = self.sampling_weights[self.positive_pixels].contiguous()
        return True

    def _frame_config(self):
        """include/vsrd_hip.h::vsrd_frame_config of this loop (one frame: the batch fields are set by whoever launches)."""
        cfg, inp, det = self.config, self.inputs, self.detector
        V, N = self.view_capacity, self.capacity       # (a row with a header: the capacities; the frame's own counts are in the header)
        w = cfg.loss_weights
        group = self.optimizer.param_groups[0]         # the box tensors' Adam constants
        return _lib.make_frame_config(N, V, inp.image_size, 1.0e-6, det.location_range, det.dimension_range, num_steps=cfg.num_steps,
                                      temperatures=(cfg.max_sdf_union_temperature, cfg.min_sdf_union_temperature),
                                      std_deviations=(cfg.max_sdf_std_deviation, cfg.min_sdf_std_deviation),
                                      loss_weights=(w["iou_projection_loss"], w["l1_projection_loss"], w["silhouette_loss"]),
                                      betas=group["betas"], adam_epsilon=group["eps"], lr_gamma=cfg.lr_gamma)

    # ---- fused glue (csrc/frame_step.h) ---------------------------------------------------------------------------------
    def _init_fused_glue(self):
        cfg, dev = self.config, self.device
        self._frame = self._frame_config()
        b = self._glue = {}
        tables = self._input_tables()
        self._full.update(tables)
        self._set_views(self.num_views)         # (the glue's tables and b["masks"]: the first V views of the full buffers)
        # (a frame of a batch: everything below lives in the frame's row of the arena, every per-instance buffer laid out for the capacity)
        declared = _glue_buffers(self.view_capacity, self.capacity, cfg, self._headed)[len(tables):]
        after_state = [name for name, *_ in declared].index("hyper_workspace")
        b.update(self._buffers(declared[:after_state]))
        if self._headed:
            self._write_header()
        self.fused_hypernetwork = True
        self.rebind()
        b.update(self._buffers(declared[after_state:]))
        # the three things a step needs before its render launch -- its rays, the boxes' side (prologue) and the generated MLP weights --
        # do not depend on each other: they run as three branches (two side streams, forked from and joined to the step's stream), and
        # so do the two things after it (epilogue, hypernetwork backward).  Captured, they become parallel branches of the hipGraph
        self._branches = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
        if cfg.scalar_interval > 0 or cfg.checkpoint_interval > 0:
            self._init_log()

    # ---- the photometric term (csrc/frame_photometric.h; scripts/main.py:689-853) ------------------------------------------------------
    def _init_photometric(self):
        """The term's buffers, at construction and only when it is live (a loop without it has none of them): the gray planes, the target
        view's hard-mask union as sampling weights with its ray table (graph mode), the drawn rays, and for the fused glue the workspace and
        outputs of vsrd_frame_photometric -- all by the one placement rule (`_new`)."""
        H, W = (int(x) for x in self.inputs.image_size)
        p = self._photometric = dict(table=None)
        p.update(self._buffers(_photometric_buffers(self.view_capacity, self.capacity, H, W, self.config, self.fused_glue)))
        if not self._write_photometric():
            raise UnsuitableFrameError("the hard masks of this frame's target view do not suit the table sampler (rendering.RayTable.suits): it "
                                       "cannot found a frame slot -- optimise it in a loop of its own (persistent=False)")

    def _write_photometric(self):
        """What the term keeps of the CURRENT frame (construction and every reset()): the gray planes of its images (vsrd_grayscale_images,
        once per frame) and the hard-mask union of view 0, soft_masks[0].amax(-1) > 0.5, taken from the row's own masks, as the weights of
        the term's draw; graph mode (re)builds their ray table in place.  False: the weights do not suit the table sampler a slot's graphs
        were captured with."""
        cfg, p, V, N = self.config, self._photometric, self.num_views, self.num_instances
        H, W = (int(x) for x in self.inputs.image_size)
        images = self.inputs.images.to(device=self.device, dtype=torch.float32).contiguous()
        _lib.check(_lib.load().vsrd_grayscale_images(_lib.ptr(images), V, H, W, _lib.ptr(p["gray"]), _lib.stream()))
        p["hard_weights"].copy_(self.flat_masks[:H * W, :N].amax(dim=-1) > 0.5)
        if self.persistent and int(p["hard_weights"].sum()) < int(cfg.surface_num_rays):
            # (a frame from a pack, whose hard pixels _check_photometric could not count: a draw would be padded with -1.  The caller
            #  optimises it in a loop of its own, whose construction says why it cannot be)
            return False
        if not (self.graph and self.device.type == "cuda"):
            return True
        had_table = p["table"] is not None
        if had_table:
            p["table"].rebuild(p["hard_weights"])
        table = p["table"] if had_table else rendering.RayTable(p["hard_weights"], allocate=None if self._row is None else self._row.bytes)
        if table.suits(int(cfg.surface_num_rays)):
            p["table"] = table
            return True
        # (as for the step's own rays, _prepare_sampler: a slot's graphs are captured with ONE sampler; a loop of one frame keeps vsrd_sample_rays)
        return not (had_table or self.persistent)

    def _draw_surface_rays(self):
        """Graph mode's draw of the term's rays (pixel indices of the target view) from the hard-mask union, keyed by (seed + 2, step counter)."""
        cfg, p = self.config, self._photometric
        if p["table"] is not None:
            return p["table"].sample(int(cfg.surface_num_rays), seed=cfg.seed + 2, stream_offset=self.step_tensor, out=p["ray_indices"])
        return rendering.sample_rays(p["hard_weights"], int(cfg.surface_num_rays), seed=cfg.seed + 2, stream_offset=self.step_tensor, out=p["ray_indices"])

    def _surface_rays(self, surface_ray_indices):
        """The term's rays of this step: the caller's (parity runs), or a draw -- torch.multinomial on the hard-mask union in the eager loop
        (the reference's stream, main.py:700-705), the device sampler in graph mode."""
        if surface_ray_indices is not None:
            return surface_ray_indices.contiguous()
        if self.graph:
            return self._draw_surface_rays()
        return torch.multinomial(self._photometric["hard_weights"], int(self.config.surface_num_rays), replacement=False)

    def _photometric_loss(self, block, surface_ray_indices):
        """The term as the autograd composition (the eager loop's; the fused call's parity reference): the target view's rays traced against
        the HARD union of the step's field block, one Newton step, the attached normals, the patch correlation (main.py:747-851)."""
        cfg, p = self.config, self._photometric
        indices = self._surface_rays(surface_ray_indices)
        hard = fields.FieldBlock(block.instances, block.temperature, block.mlp_weights, None, hard=True, yaw_gradients=block.yaw_gradients)
        directions = self.ray_directions[indices]
        positions, converged = rendering.sphere_tracing(hard, self.camera_positions[0], directions, cfg.surface_num_iterations, cfg.surface_convergence_criteria,
                                                        bounding_radius=cfg.surface_bounding_radius, initialization=False, differentiable=True)
        normals = rendering.surface_normal(hard, positions)
        V = self.num_views
        return losses.patch_correlation_loss(p["gray"][:V], self.inputs.intrinsic_matrices.to(self.device), self.inputs.extrinsic_matrices.to(self.device),
                                             indices, positions, normals, converged, tuple(cfg.surface_patch_size), int(cfg.surface_top_k))

    def _launch_photometric(self, field, surface_ray_indices, stream, frames=None, header=None):
        """vsrd_frame_photometric on the step's field, after the render launch has written grad_instances / grad_mlp and before anything reads them.
        ``frames = (B, stride)``: this loop is frame 0 of a batch -- the batched draw (every frame from its own table, keyed by its own step
        counter) and vsrd_frame_photometric_with_header with the batch's `header`, each ONE call for the B frames."""
        cfg, b, p, lib = self.config, self._glue, self._photometric, _lib.load()
        H, W = (int(x) for x in self.inputs.image_size)
        weights = cfg.loss_weights
        pw, ph = (int(x) for x in cfg.surface_patch_size)
        if frames is not None:
            if surface_ray_indices is not None or p["table"] is None:
                raise RuntimeError("a batch of frames draws the photometric term's rays from the frames' hard-mask tables")
            rays, table = int(cfg.surface_num_rays), p["table"]
            _lib.check(lib.vsrd_sample_rays_table_frames(table.table.data_ptr(), table.count, rays, (cfg.seed + 2) & 0xFFFFFFFFFFFFFFFF,
                                                         self.step_tensor.data_ptr(), p["ray_indices"].data_ptr(), int(frames[0]), int(frames[1]), stream))
            # (under a header the by-value counts are the capacities; the frames' own are in their headers)
            patch = _lib.PatchCorrelationConfig(self.view_capacity if header is not None else self.num_views, rays, H, W, pw, ph, int(cfg.surface_top_k), 0,
                                                1.0e-6, 1.0e-12)
            config = _lib.FramePhotometricConfig(int(cfg.surface_num_iterations), float(cfg.surface_convergence_criteria), float(cfg.surface_bounding_radius),
                                                 photometric_weight(cfg) / float(weights["silhouette_loss"]), int(frames[0]), int(frames[1]))
            _lib.check(lib.vsrd_frame_photometric_with_header(
                config, patch, field, _lib.ptr(self.camera_positions), _lib.ptr(self.ray_directions), _lib.ptr(p["gray"]), _lib.ptr(b["intrinsics"]),
                _lib.ptr(b["extrinsics"]), p["ray_indices"].data_ptr(), p["workspace"].data_ptr(), p["workspace"].numel(), _lib.ptr(p["loss"]),
                _lib.ptr(p["stats"]), _lib.ptr(p["grad_instances"]), _lib.ptr(p["grad_mlp"]), _lib.ptr(b["grad_instances"]), _lib.ptr(b["grad_mlp"]),
                None, None, None, header, stream))
            return
        indices = self._surface_rays(surface_ray_indices)
        rays = int(indices.numel())
        if rays != int(cfg.surface_num_rays):
            raise ValueError(f"surface_ray_indices: config.surface_num_rays = {cfg.surface_num_rays} rays (the term's buffers are laid out for them), got {rays}")
        patch = _lib.PatchCorrelationConfig(self.num_views, rays, H, W, pw, ph, int(cfg.surface_top_k), 0, 1.0e-6, 1.0e-12)
        config = _lib.FramePhotometricConfig(int(cfg.surface_num_iterations), float(cfg.surface_convergence_criteria), float(cfg.surface_bounding_radius),
                                             photometric_weight(cfg) / float(weights["silhouette_loss"]), 1, 0)
        _lib.check(lib.vsrd_frame_photometric(config, patch, field, _lib.ptr(self.camera_positions), _lib.ptr(self.ray_directions), _lib.ptr(p["gray"]),
                                              _lib.ptr(b["intrinsics"]), _lib.ptr(b["extrinsics"]), indices.data_ptr(), p["workspace"].data_ptr(),
                                              p["workspace"].numel(), _lib.ptr(p["loss"]), _lib.ptr(p["stats"]), _lib.ptr(p["grad_instances"]),
                                              _lib.ptr(p["grad_mlp"]), _lib.ptr(b["grad_instances"]), _lib.ptr(b["grad_mlp"]), None, None, None, stream))

    # ---- the device-side log (csrc/frame_log.h) -----------------------------------------------------------------------------------------
    def _init_log(self):
        """The log's buffers, at construction (a frame of a batch: in its row, the same offsets in every row): history
        [num_steps // scalar_interval, 22], snapshots [num_steps // checkpoint_interval, slot], the slots' steps, the four counters, the
        list of the five rate pointers and the segment table."""
        cfg = self.config
        rows, slots, slot_floats = _log_capacity(self.capacity, cfg)
        segments = len(_log_slot_layout(self.detector, self.hyper_distance_field, self.capacity))
        log = self._log = dict(rows=rows, slots=slots, slot_floats=slot_floats, metrics=False, masks=False)
        log.update(self._buffers(_log_buffers(self.capacity, cfg)))
        log["config"] = _lib.FrameLogConfig(
            int(cfg.scalar_interval), int(cfg.checkpoint_interval), rows, slots, slot_floats, segments, 1, 0, self.step_tensor.data_ptr(),
            self._glue["record"].data_ptr(), log["rate_pointers"].data_ptr(), self.schedule.data_ptr(), None, log["table"].data_ptr(),
            log["history"].data_ptr(), log["snapshots"].data_ptr(), log["snapshot_steps"].data_ptr(), log["counters"].data_ptr())
        self._write_log_table()

    def _write_log_table(self):
        """The frame's own pointer list and segment table: the CURRENT tensors of the modules and the optimiser (rebind() calls this again),
        the frame's own n instances at offsets laid out for the capacity, and the metrics / masks sources once log_outputs() has made them."""
        log = self._log
        log["rate_pointers"].copy_(torch.tensor([group["lr"].data_ptr() for group in self.optimizer.param_groups], dtype=torch.int64))
        sources = {"summary": self._outputs["metrics"]["summary"] if log["metrics"] else None,
                   "counts": self._outputs["masks"]["counts"][:self.num_instances] if log["masks"] else None}
        table, offset = (_lib.LogSegment * _lib.FRAME_LOG_SEGMENTS)(), 0
        log["layout"] = []
        for index, (name, tensor, size) in enumerate(_log_slot_layout(self.detector, self.hyper_distance_field, self.capacity)):
            tensor = sources[name] if tensor is None else tensor.data
            if tensor is not None:
                if not tensor.is_contiguous() or tensor.element_size() != 4 or tensor.numel() > size:
                    raise ValueError(f"{name}: a snapshot segment is a contiguous tensor of 32-bit words within its {size} reserved")
                table[index] = _lib.LogSegment(tensor.data_ptr(), tensor.numel(), offset)
            log["layout"].append((name, offset, None if tensor is None else (tuple(tensor.shape), tensor.dtype)))
            offset += size
        log["table"].copy_(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8))
        log["config"].summary = sources["summary"].data_ptr() if log["metrics"] else None

    def log_outputs(self, metrics=False, masks=False):
        """What the log reads of the other outputs from now on: with ``metrics`` the summary of vsrd_frame_metrics -- launched before every
        log launch; a frame without ``boxes_3d`` gets the summary of no pair, count 0, which names no metric -- goes into every history row and snapshot; with ``masks`` the pixel counts of
        vsrd_frame_masks (view 0) -- launched before the log launch at checkpoint boundaries -- go into every snapshot (``mask_iou``).
        Creates those outputs' buffers now (a FrameBatch: in every row, FrameBatch.log_outputs)."""
        if self._log is None:
            raise RuntimeError("log_outputs(): this loop keeps no log (OptimizationConfig.scalar_interval / checkpoint_interval)")
        for name, wanted in (("metrics", metrics), ("masks", masks)):
            if wanted:
                self._output_state(name)
            self._log[name] = bool(wanted)
        with _capture_lock, torch.no_grad():
            self._write_log_table()

    def _require_log(self, what, interval):
        if self._log is None or interval <= 0:
            raise RuntimeError(f"{what}(): this loop does not log it (OptimizationConfig.scalar_interval / checkpoint_interval)")
        return self._log

    def history(self):
        """The scalars logged so far, one row per ``scalar_interval`` steps, as device tensors sliced to the rows written (views of the
        log's buffer; the row count follows from the step count, nothing is read back): steps [rows] int32, the five losses by name
        (``eikonal_loss`` NaN for box-only steps, as the reference's dictionary has no such key then), learning_rates [rows,5] AFTER the
        step's decay (``param_group["lr"]`` when main.py logs it), hyperparameters [rows,3] = (sdf_union_temperature, sdf_std_deviation,
        cosine_ratio) of the step, metrics [rows,8] (the summary of ``metrics()`` on the parameters after the step's update; NaN when
        log_outputs(metrics=True) was not asked for)."""
        cfg = self.config
        log = self._require_log("history", cfg.scalar_interval)
        rows = min(self.step_index // cfg.scalar_interval, log["rows"])
        table = log["history"][:rows]
        steps = table[:, 0].view(torch.int32)
        result = dict(steps=steps, learning_rates=table[:, 6:11], hyperparameters=table[:, 11:14], metrics=table[:, 14:22])
        for column, name in enumerate(LOG_LOSSES, start=1):
            result[name] = table[:, column]
        result["eikonal_loss"] = torch.where(steps >= cfg.warmup_steps, table[:, 4], torch.full_like(table[:, 4], float("nan")))
        return result

    def snapshots(self):
        """The snapshots taken so far, one per ``checkpoint_interval`` steps: a list of dictionaries -- step (the tensor snapshot_steps[slot],
        int32), models (state dicts in the layout ``formats.checkpoint_payload`` gives ``models``: the parameters AFTER that step's Adam
        update, as the reference's step_{s}.pt holds them; views of the slot) and metrics (the slot's summary [8], a view, and, with masks,
        mask_iou [n] -- the slot holds the int32 pixel counts [n,3] that vsrd_frame_masks wrote, no device buffer holds an IoU, so this one
        tensor is computed from the slot's counts here, by the ``mask_iou`` function that ``masks()`` uses; an empty dictionary without either)."""
        cfg = self.config
        log = self._require_log("snapshots", cfg.checkpoint_interval)
        result = []
        for slot in range(min(self.step_index // cfg.checkpoint_interval, log["slots"])):
            words = log["snapshots"][slot]
            models = {"detector": {}, "hyper_distance_field": {}}
            metrics = {}
            for name, offset, source in log["layout"]:
                if source is None:
                    continue
                shape, dtype = source
                value = words[offset:offset + math.prod(shape)].view(dtype).view(shape)
                if name == "summary":
                    metrics["summary"] = value
                elif name == "counts":
                    metrics["mask_iou"] = mask_iou(value)
                else:
                    module, key = name.split(".", 1)
                    models[module][key] = value
            for module, key, value in [("detector", k, v) for k, v in self.detector.named_buffers()] + \
                                      [("hyper_distance_field", k, v) for k, v in self.hyper_distance_field.named_buffers()]:
                models[module][key] = value
            result.append(dict(step=log["snapshot_steps"][slot], models=models, metrics=metrics))
        return result

    # ---- the tensors whose addresses the kernels and the captured graphs hold ----------------------------------------------------
    def _bound_tensors(self):
        """Every tensor of the MODULES and the OPTIMISER whose address is handed to a kernel as a raw pointer (adam_state_tensors,
        hypernetwork_tensors, the prologue's parameter pointers): parameters, Adam's moments and counters, the learning rates.  (The
        frame's own buffers -- self._glue, step_tensor, schedule -- are created once and never replaced.)"""
        tensors = []
        for group, params in zip(self.optimizer.param_groups, self._module_parameters()):
            tensors.append(group["lr"])
            for p in params:
                state = self.optimizer.state.get(p, {})
                tensors += [p, state.get("exp_avg"), state.get("exp_avg_sq"), state.get("step")]
        return tensors

    def _module_parameters(self):
        """The modules' CURRENT parameters in the order of the optimiser's groups (__init__)."""
        det = self.detector
        return [[det.locations], [det.dimensions], [det.orientations], [det.embeddings], list(self.hyper_distance_field.parameters())]

    def rebind(self):
        """(Re)build the pointer blocks the kernels read -- Adam's state for the box tensors, the hypernetwork's parameter / moment /
        counter / rate pointers -- from the CURRENT tensors of the modules and the optimiser, and drop the captured graphs (they hold
        the old addresses).  Called at construction and, through `_check_bindings`, by itself whenever a tensor was replaced behind
        the loop's back: `optimizer.load_state_dict(...)` (new moment tensors; learning rates possibly plain floats again),
        `module.to(...)`, `load_state_dict(assign=True)`.  Adam's state is created as torch.optim.Adam(capturable=True) lays it out
        (torch creates it lazily at a parameter's first step): the kernels update these tensors in place, so checkpoints and
        optimizer.state_dict() see them like any other state."""
        cfg, det = self.config, self.detector
        for group, params in zip(self.optimizer.param_groups, self._module_parameters()):
            # load_state_dict(assign=True) swaps the parameter OBJECTS of a module: the optimiser follows them, state included
            for old, new in zip(group["params"], params):
                if old is not new and old in self.optimizer.state:
                    self.optimizer.state[new] = self.optimizer.state.pop(old)
            group["params"] = list(params)
        for group in self.optimizer.param_groups:        # a loaded state dict may carry float rates: graph mode decays device tensors in place
            lr = group["lr"]
            if not (isinstance(lr, torch.Tensor) and lr.device == self.device and lr.dtype == torch.float32):
                group["lr"] = torch.as_tensor(float(lr), dtype=torch.float32, device=self.device).clone()
            for p in group["params"]:
                state = self.optimizer.state.get(p)
                if state and not (isinstance(state.get("step"), torch.Tensor) and state["step"].device == self.device and state["step"].dtype == torch.float32):
                    state["step"] = torch.as_tensor(float(state["step"]), dtype=torch.float32, device=self.device).clone()
        self._adam = [adam_state_tensors(self.optimizer, p, group, self._row, self.capacity)
                      for group, p in zip(self.optimizer.param_groups[:3], (det.locations, det.dimensions, det.orientations))]
        # the hypernetwork and the embeddings (residual phase) run through csrc/hypernetwork.h on the same footing: torch's module
        # owns the parameters, torch.optim.Adam owns the moments and counters, the kernels update both in place
        self._hypernetwork = hypernetwork_tensors(self.hyper_distance_field, det.embeddings, self.optimizer, cfg.lr_gamma, self._row, self.capacity)
        _destroy_graphs(self._graphs)
        # references keep every bound tensor alive until the next rebind: a replaced tensor's memory is not handed to somebody else
        # while a graph that writes through its address may still be replayed
        self._bound = self._bound_tensors()
        self._bound_signature = tuple(t.data_ptr() for t in self._bound)
        if getattr(self, "_log", None) is not None:
            self._write_log_table()

    def _check_bindings(self):
        """Before anything is launched or replayed: are the tensors the pointer blocks were built from still the ones the modules and
        the optimiser hold?  (A tuple compare of ~130 addresses, ~10 us.)  If not, rebind -- the loop continues on the new tensors."""
        if not self.fused_glue:
            return
        current = self._bound_tensors()
        # (a loaded state dict may hold plain floats where the loop keeps device tensors, or lack a parameter's state: both rebind)
        if (len(current) != len(self._bound) or not all(isinstance(t, torch.Tensor) for t in current)
                or tuple(t.data_ptr() for t in current) != self._bound_signature):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("a tensor bound to the captured step was replaced during stream capture")
            if self._row is not None:
                raise RuntimeError("a parameter, moment, counter or rate of a batch frame was REPLACED (load_state_dict, module.to, assign=True): "
                                   "the frames of a FrameBatch keep them at fixed offsets of the batch's arena -- copy_ into the existing tensors")
            with _capture_lock:                          # (a device-wide synchronisation is refused while another frame's thread captures)
                torch.cuda.synchronize(self.device)      # replays that still write through the old addresses finish first
            self.rebind()

    def _fused_step(self, ray_indices, count=True, joins=(True, True), frames=None, surface_ray_indices=None):
        """One step with the box-side glue in frame_step.h.  Same arithmetic as `_step_in_scope` (the eager torch path is its
        parity reference: tests/test_hip_step.py).  ``frames = (B, stride)``: this loop is frame 0 of a batch (``FrameBatch``) and
        every launch of the step covers the B frames whose buffers lie ``stride`` bytes apart (include/vsrd_hip.h, "frame batches")."""
        cfg, b, lib, frame = self.config, self._glue, _lib.load(), self._frame
        batch = (1, 0) if frames is None else (int(frames[0]), int(frames[1]))
        frame.num_frames, frame.frame_stride = batch
        self._hypernetwork.num_frames, self._hypernetwork.frame_stride = batch
        det = self.detector
        N = self.capacity               # (the stride of every per-instance buffer; a mixed batch's row carries its own count in its header)
        residual = self.step_index >= cfg.warmup_steps
        # every launch goes through the *_with_header entry point: the plain one is its forward with a null header (csrc/api.hip)
        header = b["header"].data_ptr() if "header" in b else None          # (a row with a header: FrameBatch(max_instances=..., max_views=...))
        main = torch.cuda.current_stream(self.device)
        stream = _lib.stream()
        rays_branch, net_branch = self._branches
        fused_net = residual and self.fused_hypernetwork
        sampled = ray_indices is None
        # the draw rides in the prologue's launch (a second workgroup): no branch, no join
        with_prologue = sampled and self.ray_table is not None and getattr(self, "_prologue_draws", True)
        if batch[0] > 1 and not (with_prologue and (fused_net or not residual)):
            raise RuntimeError("a batch of frames draws its rays from the frames' sampling tables inside the prologue launch and runs the "
                               "hypernetwork through csrc/hypernetwork.h")
        if sampled and not with_prologue:   # branch 1: this step's rays (device sampler keyed by the step counter, ray_sampling.h)
            rays_branch.wait_stream(main)
            with torch.cuda.stream(rays_branch):
                self._draw_rays(b["ray_indices"], b["picks"])
        if sampled:
            ray_indices = b["ray_indices"]
        if fused_net:                   # branch 2: embeddings -> MLP weights
            hyper_ws = b["hyper_workspace"]
            if joins[0]:                # (inside a several-step graph the branch simply continues behind the hypernetwork backward of the step
                net_branch.wait_stream(main)     # before: nothing on the main stream concerns it until this step's render adjoint)
            with torch.cuda.stream(net_branch):
                _lib.check(lib.vsrd_hypernetwork_forward_with_header(self._hypernetwork, hyper_ws.data_ptr(), hyper_ws.numel(), _lib.ptr(b["mlp_weights"]),
                                                                     _lib.ptr(b["mlp_centred"]), header, _lib.stream()))
        prologue_args = (frame, _lib.ptr(det.locations.data), _lib.ptr(det.dimensions.data), _lib.ptr(det.orientations.data),
                         _lib.ptr(b["extrinsics"]), _lib.ptr(b["intrinsics"]), _lib.ptr(b["gt_boxes"]), b["visible"].data_ptr(),
                         self.step_tensor.data_ptr(), b["scratch"].data_ptr(), b["scratch"].numel(), _lib.ptr(b["instances"]),
                         b["pd_indices"].data_ptr(), b["gt_indices"].data_ptr(), b["target_columns"].data_ptr(),
                         _lib.ptr(b["instance_weights"]), _lib.ptr(self.schedule), _lib.ptr(b["projection_losses"]), _lib.ptr(b["grad_raw"]))
        if with_prologue:
            table = self.ray_table
            # (by value: the count the table's allocation is sized for -- under a header each frame's own count is its header's num_pixels;
            #  without one the two are equal, RayTable.__init__: a loop without a header never rebuilds with another count.  The table
            #  covers every pixel: no remap)
            code = lib.vsrd_frame_prologue_sample_with_header(*prologue_args, table.table.data_ptr(), table.capacity, cfg.num_rays,
                                                              (cfg.seed + 1) & 0xFFFFFFFFFFFFFFFF, None, b["ray_indices"].data_ptr(), header, stream)
            if code == _lib.E_UNSUPPORTED and header is None and batch[0] == 1 and not torch.cuda.is_current_stream_capturing():
                # the combined launch needs ~125 KB of LDS in one workgroup (cost matrix + the sampler's hash table): where that opt-in is
                # refused (and only then: a failed launch is an error), the frame keeps the bit-identical two-launch form
                # (tests: test_frame_prologue_matches_the_torch_path)
                import warnings
                warnings.warn("vsrd_frame_prologue_sample: the LDS opt-in of the combined launch was refused; this frame draws its rays "
                              "in a launch of their own (vsrd_frame_prologue + vsrd_sample_rays_table)", RuntimeWarning)
                self._prologue_draws = False
                _lib.check(lib.vsrd_frame_prologue_with_header(*prologue_args, None, stream))
                self._draw_rays(b["ray_indices"], b["picks"])
            else:
                _lib.check(code)
        else:
            _lib.check(lib.vsrd_frame_prologue_with_header(*prologue_args, header, stream))
        if sampled and not with_prologue:
            main.wait_stream(rays_branch)
        if fused_net:
            main.wait_stream(net_branch)
        ray_indices = ray_indices.contiguous()
        R = int(ray_indices.numel())
        weights = cfg.loss_weights
        eikonal_ratio = weights["eikonal_loss"] / weights["silhouette_loss"] if residual else 0.0
        from .rendering import renderers
        flags = (renderers._base_flags() & ~_lib.FLAG_MLP_SPLIT_BF16) | _lib.FLAG_YAW_GRADIENTS      # (the prologue decodes rotation_matrix_y; the epilogue reads r00, r02, r20, r22 only)
        if residual and cfg.mlp_split_bf16:
            flags |= _lib.FLAG_MLP_SPLIT_BF16
        mlp_weights = centred = None
        if fused_net:
            centred = b["mlp_centred"]
            flags |= _lib.FLAG_MLP_WEIGHTS_CENTRED
        elif residual:            # A/B: the hypernetwork through torch (rocBLAS GEMMs, autograd, torch.optim.Adam)
            self.optimizer.zero_grad(set_to_none=True)
            mlp_weights = self.hyper_distance_field(det.embeddings)[0].contiguous()          # [N,1617]
            centred = renderers._centre_mlp(mlp_weights)
            flags |= _lib.FLAG_MLP_WEIGHTS_CENTRED
        elif cfg.skip_exact_misses:
            flags |= _lib.FLAG_SKIP_EXACT_MISSES
        workspace = self.workspace.adjoint(self.device, N, residual, step_shape=(cfg.num_samples, R))
        field = _lib.make_field(b["instances"], 1.0, centred)          # (the temperature comes from the device schedule)
        config = _lib.make_config(R, cfg.num_samples, cfg.distance_range, 1.0, 1.0, 1.0e-6, 3, seed=cfg.seed, stream_offset=self.step_tensor, flags=flags,
                                  schedule=self.schedule, gather=(ray_indices, self.pixels_per_view, b["target_columns"], N), frames=frames,
                                  adjoint_slots_per_item=cfg.mlp_adjoint_item_slots if residual else 0)
        loss_scale = 1.0 / (R * self.num_instances)
        if residual:
            _lib.check(lib.vsrd_render_residual_step_with_header(field, config, _lib.ptr(self.camera_positions), _lib.ptr(self.ray_directions), None, None,
                                                                 _lib.ptr(b["masks"]), _lib.ptr(b["instance_weights"]), loss_scale, float(eikonal_ratio),
                                                                 workspace.data_ptr(), workspace.numel(), _lib.ptr(b["render_losses"]),
                                                                 _lib.ptr(b["grad_instances"]), _lib.ptr(b["grad_mlp"]), None, header, stream))
        else:
            _lib.check(lib.vsrd_render_silhouette_step_with_header(field, config, _lib.ptr(self.camera_positions), _lib.ptr(self.ray_directions), None, None,
                                                                   _lib.ptr(b["masks"]), _lib.ptr(b["instance_weights"]), loss_scale,
                                                                   workspace.data_ptr(), workspace.numel(), _lib.ptr(b["render_losses"]),
                                                                   _lib.ptr(b["grad_instances"]), None, header, stream))
        photometric = residual and self._photometric is not None
        if photometric:
            # on the step's own stream: the call ends in the accumulation into grad_instances / grad_mlp, which the render launch has just
            # written and which the hypernetwork's backward and the epilogue read next -- no stretch of it is free of both
            self._launch_photometric(field, surface_ray_indices, stream, frames=None if frames is None else batch, header=header)
        if fused_net:     # branch: backward through the hypernetwork, Adam on it and on the embeddings, both rates decayed (next to the epilogue)
            net_branch.wait_stream(main)
            with torch.cuda.stream(net_branch):
                _lib.check(lib.vsrd_hypernetwork_backward_step_with_header(self._hypernetwork, hyper_ws.data_ptr(), hyper_ws.numel(), _lib.ptr(b["grad_mlp"]),
                                                                           float(weights["silhouette_loss"]), header, _lib.stream()))
        groups = self.optimizer.param_groups
        # ExponentialLR decays every group's rate AFTER the optimiser step: the epilogue does it for the groups it steps itself (and, in
        # the box-only phase, for the two that have nothing to step); in the residual phase those two are decayed after torch's step
        others = (None, None) if residual else (_lib.ptr(groups[3]["lr"]), _lib.ptr(groups[4]["lr"]))
        epilogue_args = (frame, _lib.ptr(b["grad_instances"]), _lib.ptr(b["grad_raw"]), _lib.ptr(b["projection_losses"]), _lib.ptr(b["render_losses"]),
                         float(eikonal_ratio), self._adam[0], self._adam[1], self._adam[2], others[0], others[1], self.step_tensor.data_ptr(),
                         _lib.ptr(b["record"]), _lib.ptr(b["raw_gradients"]))
        _lib.check(lib.vsrd_frame_epilogue_with_header(*epilogue_args, header, stream))
        if photometric:   # record[4], which the epilogue has just written, gains the term
            p = self._photometric
            if frames is None:
                _lib.check(lib.vsrd_frame_photometric_finish(_lib.ptr(p["loss"]), _lib.ptr(p["stats"]), photometric_weight(cfg), _lib.ptr(b["record"]), stream))
            else:
                _lib.check(lib.vsrd_frame_photometric_finish_with_header(_lib.ptr(p["loss"]), _lib.ptr(p["stats"]), photometric_weight(cfg),
                                                                         _lib.ptr(b["record"]), *batch, stream))
        if residual and not fused_net:    # autograd + torch.optim.Adam (the box tensors have no .grad: skipped)
            mlp_weights.backward(b["grad_mlp"] * weights["silhouette_loss"])
            self.optimizer.step()
            groups[3]["lr"].mul_(cfg.lr_gamma)
            groups[4]["lr"].mul_(cfg.lr_gamma)
        if fused_net and joins[1]:
            main.wait_stream(net_branch)
        if count:
            self.step_index += 1
        return self._step_record(residual)

    def _step_record(self, residual):
        """The dictionary a fused step returns: views of the record the epilogue writes (device tensors, rewritten by every step);
        `residual`: the step ran in the residual phase and has an eikonal term."""
        record, raw = self._glue["record"], self._glue["raw_gradients"][:self.num_instances]
        result = dict(iou_projection_loss=record[0], l1_projection_loss=record[1], silhouette_loss=record[2], loss=record[4],
                      raw_gradients=[raw[:, 0:3].unsqueeze(0), raw[:, 3:6].unsqueeze(0), raw[:, 6:8].unsqueeze(0)])
        if residual:
            result["eikonal_loss"] = record[3]
            if self._photometric is not None:
                result["photometric_loss"] = self._photometric["loss"][0]
        return result

    # ------------------------------------------------------------------------------------------------
    def sample_rays(self):
        """main.py:620-627: importance-sample rays by the strongest soft mask (torch.multinomial, no replacement).  Graph mode
        uses the library's own sampler (same algorithm, Philox keyed by the device-side step counter): ATen's captured multinomial
        faults on replay with this torch build, and it sorts all V*H*W keys every step."""
        if self.graph:
            return self._draw_rays(torch.empty(self.config.num_rays, dtype=torch.int64, device=self.device))
        return torch.multinomial(self.sampling_weights, self.config.num_rays, replacement=False)

    def _draw_rays(self, out, picks=None):
        """Graph mode's draw of this step's rays into `out` (pixel indices over all views), keyed by the device-side step counter."""
        cfg = self.config
        if self.ray_table is not None:
            return self.ray_table.sample(cfg.num_rays, seed=cfg.seed + 1, stream_offset=self.step_tensor, out=out, remap=self.ray_remap)
        picks = rendering.sample_rays(self.positive_weights, cfg.num_rays, seed=cfg.seed + 1, stream_offset=self.step_tensor, out=picks)
        return torch.index_select(self.positive_pixels, 0, picks, out=out)

    def field_block(self, outputs, temperature, mlp_weights=None):
        return fields.FieldBlock(fields.pack_instances(outputs["locations"][0], outputs["orientations"][0], outputs["dimensions"][0]),
                                 float(temperature), mlp_weights, None, yaw_gradients=True)      # (BoxParameters3D: rotation_matrix_y)

    def step(self, ray_indices: Optional[torch.Tensor] = None, u_coarse=None, u_fine=None, surface_ray_indices: Optional[torch.Tensor] = None):
        """One optimisation step.  Steps < warmup_steps optimise the boxes only; later steps add the per-instance residual MLP
        (hypernetwork on the embeddings, main.py:525-578) and the eikonal loss (main.py:679-687).
        ray_indices / uniforms may be supplied for reproducible parity runs, and so may surface_ray_indices, the photometric term's rays (pixel
        indices of the target view; used by the steps in which the term is live).  With the term live the dictionary gains
        ``photometric_loss`` and ``loss`` includes it."""
        if surface_ray_indices is not None and self._photometric is None:
            raise ValueError("surface_ray_indices: the photometric term is off (loss_weights['photometric_loss'])")
        if self.graph:
            if u_coarse is not None or u_fine is not None:
                raise ValueError("graph mode draws its uniforms in the kernels (Philox keyed by the device-side step counter)")
            return self._graph_advance(1, ray_indices, surface_ray_indices)
        return self._step(ray_indices, u_coarse, u_fine, surface_ray_indices=surface_ray_indices)

    # ---- hipGraph mode ---------------------------------------------------------------------------------
    def _device_schedule(self):
        """scripts/main.py:420-431 evaluated on the device from the device-side step counter."""
        cfg = self.config
        x = self.step_tensor.to(torch.float32) / cfg.num_steps
        anneal = (torch.cos(math.pi * x) + 1.0) / 2.0
        self.schedule.copy_(torch.cat([anneal * (cfg.max_sdf_union_temperature - cfg.min_sdf_union_temperature) + cfg.min_sdf_union_temperature,
                                       anneal * (cfg.max_sdf_std_deviation - cfg.min_sdf_std_deviation) + cfg.min_sdf_std_deviation, x]))

    def _graph_advance(self, k, ray_indices=None, surface_ray_indices=None):
        """``k`` steps of graph mode (``_advance``) and what is this loop's own around them: its checks, its key -- (phase, ray source) for a
        single step, with "surface" behind it when the photometric term's rays are the caller's too, (phase, False, k) for a group -- its step
        count and its log."""
        if ray_indices is not None and int(ray_indices.numel()) > self.config.num_rays:
            # the captured graphs hold the address of scratch sized for config.num_rays rays; a larger launch would outgrow it
            raise ValueError(f"graph mode replays steps of at most config.num_rays = {self.config.num_rays} rays, got {int(ray_indices.numel())}")
        self._check_bindings()
        residual = self.step_index >= self.config.warmup_steps
        key = (residual, ray_indices is not None) if k == 1 else (residual, False, k)
        if surface_ray_indices is None:
            outputs = _advance(self, key, k, lambda rays, **how: self._step(rays, None, None, **how), static=ray_indices)
        else:
            # static rays are part of the graph's key; `_advance` keeps ONE static tensor: the step's rays (if given) and the term's, end to end
            n = 0 if ray_indices is None else int(ray_indices.numel())
            surface = surface_ray_indices.reshape(-1).to(torch.int64)
            packed = surface if n == 0 else torch.cat([ray_indices.reshape(-1).to(torch.int64), surface])
            outputs = _advance(self, (*key, "surface"), k,
                               lambda rays, **how: self._step(rays[:n] if n else None, None, None, surface_ray_indices=rays[n:], **how), static=packed)
        self.step_index += k
        _launch_log([self])
        return outputs

    def run(self, num_steps, steps_per_graph=4):
        """``num_steps`` optimisation steps, the last step's outputs returned.  In graph mode up to ``steps_per_graph`` consecutive
        steps of one phase are captured in ONE hipGraph and replayed together: between two graph launches the GPU idles for ~20 us
        (profiles/r03/native_step_timeline_residual.txt: the gap behind the last kernel of a replay), a fifth of a box-only step.  The
        steps themselves are the same launches in the same order as ``step()``'s, so the trajectory is bit-identical
        (tests/test_hip_step.py::test_run_replays_several_steps_per_graph)."""
        outputs = None
        remaining = int(num_steps)
        while remaining > 0:
            k = 1
            if self.graph and self.fused_glue:
                residual = self.step_index >= self.config.warmup_steps
                k = _steps_in_next_group(remaining, None if residual else self.config.warmup_steps - self.step_index, _steps_to_log_boundary([self]),
                                         steps_per_graph, (residual, False) in self._graphs)
            outputs = self._graph_advance(k) if k > 1 else self.step()
            remaining -= k
        return outputs

    def _step(self, ray_indices, u_coarse, u_fine, count=True, joins=(True, True), surface_ray_indices=None):
        with rendering.workspace_scope(self.workspace):
            if self.fused_glue:
                if not torch.cuda.is_current_stream_capturing():
                    self._check_bindings()
                return self._fused_step(ray_indices, count, joins, surface_ray_indices=surface_ray_indices)
            return self._step_in_scope(ray_indices, u_coarse, u_fine, count, surface_ray_indices)

    def _step_in_scope(self, ray_indices, u_coarse, u_fine, count, surface_ray_indices=None):
        cfg, inp = self.config, self.inputs
        step = self.step_index
        residual = step >= cfg.warmup_steps
        self.optimizer.zero_grad(set_to_none=True)
        outputs = self.detector()
        # ---- multi-view projection, matching, projection losses (main.py:339-415) --------------------
        pd_boxes_2d, _ = operations.project_boxes_multi_view(outputs["boxes_3d"][0], inp.extrinsic_matrices, inp.intrinsic_matrices, inp.image_size)
        pd_idx, gt_idx = losses.match_instances(pd_boxes_2d[0], inp.boxes_2d[0])
        iou_loss, l1_loss = losses.projection_losses(pd_boxes_2d, inp.boxes_2d, inp.visible_masks, pd_idx, gt_idx)
        # ---- instance loss (main.py:420-671) ---------------------------------------------------------
        ratio, temperature, std = losses.schedules(step, cfg.num_steps, cfg.max_sdf_union_temperature, cfg.min_sdf_union_temperature,
                                                   cfg.max_sdf_std_deviation, cfg.min_sdf_std_deviation)
        schedule = offset = None
        if self.graph:       # the kernels read (temperature, std, ratio) and the Philox counter from device memory instead
            self._device_schedule()
            schedule, offset = self.schedule, self.step_tensor
        mlp_weights = self.hyper_distance_field(outputs["embeddings"])[0].contiguous() if residual else None     # [N,1617]
        block = self.field_block(outputs, temperature, mlp_weights)
        if ray_indices is None:
            ray_indices = self.sample_rays()
        origins = self.camera_positions[ray_indices // self.pixels_per_view]
        directions = self.ray_directions[ray_indices]
        weights = cfg.loss_weights
        if residual:    # render + silhouette BCE + eikonal term + adjoint (boxes and MLP weights) in one launch
            eikonal_ratio = weights["eikonal_loss"] / weights["silhouette_loss"]
            rendered, parts = rendering.silhouette_step(block, origins, directions, self.flat_masks[ray_indices], cfg.distance_range,
                                                        cfg.num_samples, std, ratio, pd_indices=pd_idx, gt_indices=gt_idx,
                                                        u_coarse=u_coarse, u_fine=u_fine, seed=cfg.seed, stream_offset=step if offset is None else offset,
                                                        skip_exact_misses=False, schedule=schedule, eikonal_ratio=eikonal_ratio, return_terms=True,
                                                        mlp_split_bf16=cfg.mlp_split_bf16)
            silhouette, eikonal = parts[0], parts[1]
        else:           # box-only phase: render + silhouette BCE + adjoint in one launch
            rendered = rendering.silhouette_step(block, origins, directions, self.flat_masks[ray_indices], cfg.distance_range,
                                                 cfg.num_samples, std, ratio, pd_indices=pd_idx, gt_indices=gt_idx,
                                                 u_coarse=u_coarse, u_fine=u_fine, seed=cfg.seed, stream_offset=step if offset is None else offset,
                                                 skip_exact_misses=cfg.skip_exact_misses, schedule=schedule)
            silhouette = rendered.detach()
        terms = dict(iou_projection_loss=iou_loss, l1_projection_loss=l1_loss, silhouette_loss=silhouette)
        if residual:
            terms["eikonal_loss"] = eikonal
        # main.py:855: sum of weighted terms; `rendered` already is silhouette (+ eikonal_ratio * eikonal)
        total = weights["iou_projection_loss"] * iou_loss + weights["l1_projection_loss"] * l1_loss + weights["silhouette_loss"] * rendered
        if residual and self._photometric is not None:       # main.py:689-853, on the hard union of the step's field block
            terms["photometric_loss"] = self._photometric_loss(block, surface_ray_indices)
            total = total + photometric_weight(cfg) * terms["photometric_loss"]
        total.backward()
        raw_gradients = [p.grad.detach().clone() for p in (self.detector.locations, self.detector.dimensions, self.detector.orientations)]
        self.optimizer.step()
        if self.graph:      # ExponentialLR and the step counter, in place on the device
            for group in self.optimizer.param_groups:
                group["lr"].mul_(cfg.lr_gamma)
            self.step_tensor.add_(1)
        else:
            self.scheduler.step()
        if count:
            self.step_index += 1
        terms["loss"] = total
        result = {name: value.detach() for name, value in terms.items()}
        result["raw_gradients"] = raw_gradients
        return result

    # ---- a frame SLOT: the loop and its captured graphs, reused for frame after frame (round 5) -----------------------------------------
    def capture_all(self, steps_per_graph=4):
        """Run, NOW, every eager warm-up step and every capture a frame's ``run()`` would meet on its way -- box-only and residual phase, the
        one-step and the ``steps_per_graph``-step graph of each -- on the current frame's data, then ``reset()`` the frame.  A launcher
        does this once per slot at start-up, one slot after the other and before any worker thread exists: afterwards a frame is copies,
        fills and graph replays only, and stream capture -- a process-wide mode that every collision of round 4 had on one side -- never
        happens next to another frame's work again.  Returns the number of graphs held."""
        if not (self.graph and self.fused_glue and self.persistent):
            raise ValueError("capture_all() belongs to a persistent graph-mode loop (FrameOptimizer(..., graph=True, persistent=True))")
        k = int(steps_per_graph)
        _capture_phases([self], k, self.step, lambda: self._graph_advance(k))
        with _capture_lock:
            torch.cuda.current_stream(self.device).synchronize()
        self.reset(self.inputs)
        return len(self._graphs)

    def _copy_inputs(self, inputs, V, N):
        """reset() from a materialised FrameInputs: the strided copy into the loop's buffers and the importance weights."""
        b = self._glue
        # `inputs` may be what a reset from a frame pack left in self.inputs (_ingest_pack): its soft_masks and boxes_2d are VIEWS of this
        # loop's own buffers (capture_all ends with reset(self.inputs)).  The loop holds the frame already; copying it onto itself would be an
        # overlapping copy_, so only what is derived from it is refreshed.
        if inputs.soft_masks.data_ptr() != self.flat_masks.data_ptr():
            self.flat_masks[:, :N].copy_(inputs.soft_masks.reshape(-1, N))
            b["gt_boxes"][:, :N].copy_(inputs.boxes_2d.reshape(V, N, 4))
            b["visible"][:, :N].copy_(inputs.visible_masks)
        torch.amax(self.flat_masks[:, :N], dim=-1, out=self.sampling_weights)

    def _ingest_pack(self, pack, H, W, N):
        """reset() from a frame pack: ONE vsrd_frame_ingest call writes columns 0..N-1 of the row's soft masks (stride: the row's capacity), its
        importance weights, ground-truth boxes and visibility -- no [V,H,W,N] temporary, no strided copy, no amax.  Returns the FrameInputs
        that `self.inputs` then holds: its camera matrices are the pack's, and its soft_masks, boxes_2d are VIEWS of the row's buffers (they
        change with the row's next reset; visible_masks is a small copy)."""
        b, V = self._glue, self.num_views
        stride = int(self.flat_masks.shape[1])
        frames.ingest_into(pack, self.device, stride, soft_masks=self.flat_masks, sampling_weights=self.sampling_weights, gt_boxes=b["gt_boxes"],
                           visible=b["visible"])
        intrinsics, extrinsics = frames.camera_matrices(pack, self.device)
        return FrameInputs((H, W), intrinsics, extrinsics, self.flat_masks.view(V, H, W, stride)[..., :N],
                           b["gt_boxes"][:, :N].unflatten(-1, (2, 2)), b["visible"][:, :N].bool(), *frames.ground_truth_3d(pack, self.device),
                           **frames.group_tables(pack, self.device),
                           images=frames.pack_images(pack, self.device) if self._photometric is not None else None)

    def reset(self, inputs: FrameInputs, init_seed=None):
        """Start ANOTHER frame of the same shape in this loop, in place: the new frame's matrices, boxes and soft masks are copied into
        the buffers the captured graphs read; parameters are re-initialised as a fresh ``BoxParameters3D`` / ``HyperDistanceField`` would
        be (scripts/main.py:106-199 builds new models per frame); Adam's moments, counters and learning rates, the step counter and the
        sampling table start over.  No allocation that a graph would have to learn about, no capture.  Returns False -- and leaves the
        loop unusable for that frame -- when the frame's importance weights do not suit the table sampler the graphs were captured with
        (the caller then optimises it in a loop of its own)."""
        if not (self.graph and self.fused_glue and self.persistent):
            raise ValueError("reset() belongs to a persistent graph-mode loop (FrameOptimizer(..., graph=True, persistent=True))")
        cfg, dev, b = self.config, self.device, self._glue
        # any frame -- a pack (frames.py) or a materialised FrameInputs -- of the loop's image size; a row with a header: with 1..view capacity
        # views and 1..capacity instances, any other loop: with its own counts
        V, H, W, N = _incoming_shape(inputs, (self.num_views, *self.inputs.image_size, self.num_instances),
                                     (self.view_capacity, self.capacity) if self._headed else None)
        for output in _OUTPUTS.values():         # (before anything of the row is overwritten: the 3-D ground truth, the group)
            output.check(self, inputs, N)
        _check_photometric(inputs, cfg, V, N)
        with _capture_lock, torch.no_grad():
            main = torch.cuda.current_stream(dev)
            main.synchronize()                                      # (replays of the previous frame have finished: nothing reads the buffers)
            # ---- inputs ----
            if V != self.num_views:
                self._set_views(V)               # (the first V views of the row's buffers: the same addresses)
            if isinstance(inputs, frames.FramePack):
                # vsrd_frame_ingest writes the soft masks, importance weights, boxes and visibility in place
                inputs = self._ingest_pack(inputs, H, W, N)
            else:
                self._copy_inputs(inputs, V, N)
            b["extrinsics"].copy_(inputs.extrinsic_matrices.reshape(V, 16))
            b["intrinsics"].copy_(inputs.intrinsic_matrices.reshape(V, 9))
            cam, dirs = rendering.ray_casting((H, W), inputs.intrinsic_matrices, inputs.extrinsic_matrices)
            self.camera_positions.copy_(cam)
            self.ray_directions.copy_(dirs.reshape(-1, 3))
            self.inputs = inputs
            for name, state in self._outputs.items():
                _OUTPUTS[name].write(self, state, N)         # (the row's 3-D ground truth, its group: the new frame's, or none)
            if N != self.num_instances:
                # the detector's parameters and their moments become the first N instances of their [1, capacity, ...] buffers (same
                # addresses: the pointer blocks and the captured graphs stay valid)
                for param in (self.detector.locations, self.detector.dimensions, self.detector.orientations, self.detector.embeddings):
                    param.data = _instance_prefix(param.data, N)
                    state = self.optimizer.state.get(param)
                    if state:
                        state["exp_avg"], state["exp_avg_sq"] = _instance_prefix(state["exp_avg"], N), _instance_prefix(state["exp_avg_sq"], N)
                self.num_instances = N
                self._bound = self._bound_tensors()
            # ---- parameters, optimiser, counters ----
            with _initial_draw:                                   # (OptimizationConfig.init_seed, for THIS frame: seed and draw as one step -- the generator is the process's,
                if init_seed is not None:                         #  and the capture gate lets several frames' threads in here at once)
                    torch.default_generator.manual_seed(int(init_seed))
                fresh_modules = _fresh_modules(N)
            for module, fresh in zip((self.detector, self.hyper_distance_field), fresh_modules):
                for p, q in zip(module.parameters(), fresh.parameters()):
                    p.copy_(q)
            for group, rate in zip(self.optimizer.param_groups, _initial_rates(cfg)):
                group["lr"].fill_(rate)
                for p in group["params"]:
                    state = self.optimizer.state.get(p)
                    if state:
                        state["exp_avg"].zero_(); state["exp_avg_sq"].zero_(); state["step"].zero_()
            self.step_tensor.zero_()
            self.schedule.fill_(1.0)
            self.step_index = 0
            for name in ("record", "raw_gradients", "grad_raw", "grad_instances", "grad_mlp", "projection_losses", "render_losses"):
                b[name].zero_()
            if self._headed:
                self._write_header()
            if self._log is not None:            # (the log starts over; its table follows the frame's own instance count)
                self.log_seconds = 0.0
                self._log["counters"].zero_()
                self._log["snapshot_steps"].fill_(-1)
                self._write_log_table()
            suits = self._prepare_sampler(cfg)
            if self._photometric is not None:    # (the new frame's gray planes and hard masks, in the buffers the graphs read)
                # (ray_indices too: the draw overwrites them before use, but a slot then holds what a fresh loop -- or a batch's row -- holds
                #  in the box-only steps, which is what a state comparison between the two looks at)
                for name in ("loss", "stats", "grad_instances", "grad_mlp", "ray_indices"):
                    self._photometric[name].zero_()
                suits = self._write_photometric() and suits
            main.synchronize()
        return suits

    def boxes(self):
        with torch.no_grad():
            return self.detector()

    # ---- what a frame can be asked for after its steps (_OUTPUTS) ------------------------------------------------------------------
    def _output_state(self, name):
        """The buffers of output `name` (_OUTPUTS[name].buffers), created at first use -- in the frame's row when there is one (a
        FrameBatch creates them in every row at once: equal offsets) -- and laid out for the capacities.  What an output keeps of the
        frame among them (metrics(): its 3-D ground truth) is checked before anything is created, written here and by every reset()."""
        if name not in self._outputs:
            output = _OUTPUTS[name]
            H, W = (int(x) for x in self.inputs.image_size)
            output.check(self, self.inputs, self.num_instances)
            with _capture_lock, torch.no_grad():
                state = self._outputs[name] = self._buffers(output.buffers(getattr(self, output.leading), self.capacity, H, W))
                output.write(self, state, self.num_instances)
        return self._outputs[name]

    def _launch_output(self, name, frames=None, **arguments):
        """ONE vsrd_frame_* call on this loop's tensors; ``frames = (B, stride)``: this loop is row 0 of a batch, as in `_fused_step`."""
        state = self._output_state(name)       # (the frame config's batch fields are this call's own: a copy of the glue's)
        if not self.fused_glue and "frame" not in state:
            state["frame"] = self._frame_config()      # (a loop without the fused glue has no frame config of its own)
        frame = _lib.FrameConfig.from_buffer_copy(self._frame if self.fused_glue else state["frame"])
        frame.num_frames, frame.frame_stride = (1, 0) if frames is None else (int(frames[0]), int(frames[1]))
        header = self._glue.get("header") if self.fused_glue else None
        with _capture_lock:
            _lib.check(_OUTPUTS[name].launch(self, state, frame, None if header is None else header.data_ptr(), **arguments))
        return state

    def _take(self, name, inputs):
        """One call's own `inputs` of output `name` into its state (first use creates it), as host values: outside any capture."""
        with _capture_lock, torch.no_grad():
            _OUTPUTS[name].take(self, self._output_state(name), **inputs)

    def _ask(self, name, inputs={}, **arguments):
        """Output `name` (_OUTPUTS) of this loop: the preconditions, the call's own `inputs` (_FrameOutput.take), ONE launch on the current
        stream, the frame's own views."""
        _check_asked(name, [self])
        self._take(name, inputs)
        state = self._launch_output(name, **arguments)
        return _OUTPUTS[name].views(self, state, **arguments)

    def labels(self):
        """The frame's pseudo-labels from its CURRENT parameters (tools/kitti_360/make_predictions.py:61-192), by one vsrd_frame_labels
        launch on the current stream, no host synchronisation: a dictionary of device tensors sliced to the frame's own V views and n instances --
        boxes_3d [V,n,8,3] (camera-frame corners in every view), boxes_2d [V,n,2,2] (clipped), confidences [n] (the matched mean IoU),
        matched_gt [n], mean_iou [n,n].  They are views of buffers the next call overwrites (formats.save_frame_labels writes them out)."""
        return self._ask("labels")

    def _check_has_group(self):
        if label_view_count(self.inputs) == 0:
            raise ValueError("group_labels() needs the frame's group: FrameInputs.label_frame_ids is None")
        if self.label_view_capacity == 0:
            raise ValueError("group_labels(): this loop was laid out for no label views (max_label_views)")

    def group_labels(self):
        """The frame's pseudo-labels in the views of its GROUP (``FrameInputs.label_*``; tools/kitti_360/make_predictions.py:50-192: the frames
        whose instance set equals the target's, which are the frames a detector is trained on -- not the views the frame was optimised on,
        which ``labels()`` serves) from its CURRENT parameters, by one vsrd_frame_group_labels call on the current stream, no host
        synchronisation; like ``labels()`` it needs no step to have run.  A dictionary of device tensors sliced to the frame's own l label
        views and n instances: boxes_3d [l,n,8,3], boxes_2d [l,n,2,2], confidences [n], matched_gt [n], mean_iou [n,n], frame_ids [l].
        They are views of buffers the next call overwrites (formats.save_frame_group_labels writes them out).  ValueError when the frame has
        no group."""
        self._check_has_group()
        return self._ask("group_labels")

    def masks(self, view=0, threshold=0.5, soft=False):
        """The frame's dense predicted instance masks of view ``view`` (0: the target view) -- what the reference renders every
        ``image_intervals`` steps (scripts/main.py:1011-1061: volume_masks * surface_masks) -- by one vsrd_frame_masks launch on the current
        stream, no host synchronisation.  They render the field of the loop's `instances` (and, in the residual phase, MLP weight) buffers at
        the loop's `schedule`: the field the LAST STEP rendered, built from the parameters that step started from -- which is what the
        reference logs (main.py:1013 uses the fields built at the top of the step), not the parameters after that step's Adam update.
        RuntimeError when no step has run since construction or ``reset()``.  A dictionary of device tensors sliced to the frame's own n
        instances: inside [n,H,ceil(W/8)] uint8 (numpy.packbits along W, the frame packs' mask format), counts [n,3] int32 (#pred,
        #target, #both against the soft masks the frame was fitted to, through the last step's assignment), mask_iou [n], and with
        ``soft`` the values themselves, soft [H,W,n].  They are views of buffers the next call overwrites (formats.save_frame_masks)."""
        _check_view(view, [self], alone=True)
        return self._ask("masks", view=view, threshold=threshold, soft=soft)

    def surface(self, view=0, hard=True, light=None, shadows=True, background=None, alpha=None):
        """The dense surface render of view ``view`` (0: the target view) -- the surface of the fitted field with range, owning instance,
        shadow and a shaded image, what the dense logging branch of scripts/main.py:1028-1041 composes from sphere_tracing, surface_normal,
        shadow_rendering and phong_shading -- by one vsrd_frame_surface launch on the current stream, no host synchronisation.  It renders
        the field the LAST STEP rendered, by the rule of ``masks()``.  ``hard``: trace the hard union (the default; the reference's logging
        trace uses the soft one, ``hard=False``); ``light`` [3]: the direction the light travels (None: rendering.SURFACE_LIGHT);
        ``background`` [H,W,3] uint8: the photograph the shaded colours are laid over with weight ``alpha`` (None: 0.6 over a background,
        else 1).  RuntimeError when no step has run since construction or ``reset()``.  A dictionary of device tensors: converged_bits /
        shadow_bits [H, ceil(W/8)] uint8 (numpy.packbits along W), instance [H,W] uint8 (255: none), range [H,W], colors [H,W,3] uint8,
        light [3], shape, view.  They are views of buffers the next call overwrites (formats.save_frame_surface)."""
        _check_view(view, [self], alone=True)
        return self._ask("surface", dict(light=light, background=background), view=view, hard=hard, shadows=shadows, background=background is not None, alpha=alpha)

    def metrics(self):
        """The frame's evaluation against its 3-D ground truth (``FrameInputs.boxes_3d``) -- the reference's iou_3d, iou_bev and accuracies
        (scripts/main.py:870-924) -- by one vsrd_frame_metrics launch on the current stream, no host synchronisation.  The boxes are decoded
        from the loop's CURRENT parameters, as ``labels()`` decodes them and as a checkpoint stores them, and paired with the ground truth by
        the LAST STEP's matching (the glue's pd_indices / gt_indices); the reference logs the boxes that step started from, one Adam update
        earlier.  RuntimeError when no step has run since construction or ``reset()`` (there is no matching yet), ValueError when the
        frame has no ``boxes_3d``.  A dictionary of device tensors sliced to the frame's own n instances: iou_3d [n], iou_bev [n] (by
        prediction; NaN where the matched ground-truth slot has no annotation), summary [8] (count, iou_3d, iou_bev, accuracy_3d_25,
        accuracy_bev_25, accuracy_3d_50, accuracy_bev_50, 0: ``formats.frame_metrics`` names them), corners [n,8,3] (the decoded boxes).
        They are views of buffers the next call overwrites."""
        _check_asked("metrics", [self])          # (first, as ever: a loop that cannot be asked says so whatever its ground truth)
        if self.inputs.boxes_3d is None:
            raise ValueError("metrics() needs the frame's 3-D ground truth: FrameInputs.boxes_3d is None")
        return self._ask("metrics")

    def close(self):
        """Drop the captured graphs and the scratch buffers (also happens when the optimizer is garbage-collected).  Once per frame
        this is also where the device ray sampler's sticky overflow flag is read back (a host synchronisation, so not per step): a
        draw whose threshold bin held more candidate keys than the sampler lists was incomplete and not reproducible."""
        with _capture_lock:
            incomplete = bool(self.graph and self.ray_table is not None and self.ray_table.incomplete())
            overflowed = bool(self.graph and self.workspace.sampler_overflowed(self.device))
            dropped = self._log["counters"].tolist() if getattr(self, "_log", None) is not None else [0, 0, 0, 0]
        if dropped[1] or dropped[3]:
            import warnings
            warnings.warn(f"vsrd_frame_log dropped {dropped[1]} history rows and {dropped[3]} snapshots of this frame: it ran beyond the "
                          "capacities num_steps // interval its log was laid out for", RuntimeWarning)
        if incomplete:
            import warnings
            warnings.warn("vsrd_sample_rays_table ran out of picks in some step of this frame: those draws repeat some rays "
                          "(see csrc/ray_sampling.h and RayTable.suits)", RuntimeWarning)
        if overflowed:
            import warnings
            warnings.warn("vsrd_sample_rays overflowed its candidate list in some step of this frame: those draws were incomplete "
                          "(many equal importance weights in one histogram bin); see csrc/ray_sampling.h", RuntimeWarning)
        _destroy_graphs(self._graphs)
        self.ray_table = None                  # (43 MB per frame at the reference's size: the table and its guide)
        if getattr(self, "_photometric", None) is not None:
            self._photometric["table"] = None
        self.workspace.release()

    def __del__(self):
        try:
            _destroy_graphs(self._graphs, wait=False)
        except Exception:                      # (interpreter shutdown: module globals may be gone)
            pass

    # ---- checkpoint views (scripts/main.py:1109-1121 saves optimizer.state_dict() and scheduler.state_dict()) ----------------
    def optimizer_state_dict(self):
        """``optimizer.state_dict()`` in the layout the reference's ``torch.optim.Adam`` loads: float learning rates (graph mode
        keeps them as device tensors decayed in place), ``initial_lr`` per group as ExponentialLR records it, step counters as
        host float tensors (capturable Adam keeps them on the device)."""
        state = self.optimizer.state_dict()
        groups = []
        for group, base in zip(state["param_groups"], _initial_rates(self.config)):
            group = dict(group)
            group["lr"] = float(group["lr"])
            group.setdefault("initial_lr", base)
            group["capturable"] = False
            groups.append(group)
        per_param = {}
        for index, entry in state["state"].items():
            entry = dict(entry)
            if isinstance(entry.get("step"), torch.Tensor):
                entry["step"] = entry["step"].detach().to("cpu", torch.float32)
            per_param[index] = entry
        return dict(state=per_param, param_groups=groups)

    def scheduler_state_dict(self):
        """``ExponentialLR.state_dict()`` after ``step_index`` steps.  Graph mode has no scheduler object (the rates are decayed on
        the device inside the captured step): the same dictionary is assembled from the step counter and the device-side rates."""
        if self.scheduler is not None:
            return self.scheduler.state_dict()
        cfg = self.config
        return {"gamma": cfg.lr_gamma,
                "base_lrs": _initial_rates(cfg),
                "last_epoch": self.step_index, "_step_count": self.step_index + 1, "_is_initial": False,
                "_get_lr_called_within_step": False, "_last_lr": [float(group["lr"]) for group in self.optimizer.param_groups]}


class FrameBatch:
    """B frames of ONE shape (or, with capacities, of one image size) optimised in lock-step: every launch of a step -- prologue + ray draw, hypernetwork forward, render +
    losses + adjoint, MLP adjoint, reductions, hypernetwork backward + Adam, epilogue -- covers all B frames at once (include/vsrd_hip.h,
    "frame batches").  The reference's loop carries the same batch dimension (scripts/main.py:525-651: lists over the batch of distance
    fields, camera positions, ray directions, soft masks; BoxParameters3D(batch_size, num_instances), box_parameters.py:34-49); its
    configs use batch_size = 1 because one V100 was full with one frame -- one MI355X is not (1000 rays = one wave per SIMD).

    The frames stay INDEPENDENT problems: each has its own detector, hypernetwork, Adam state, learning rates, step counter (which keys its
    Philox streams), sampling table and scratch, in its own row of ``self.arena``; nothing is summed across frames.  A frame of a batch
    therefore walks, bit for bit, the trajectory it walks alone in a ``FrameOptimizer(graph=True, persistent=True)``
    (tests/test_hip_step.py::test_frame_batch_walks_each_frames_own_trajectory).  Each member is such a loop whose buffers live in the
    arena; the batch launches member 0's step with ``frames = (B, stride)``.

    Like a frame slot, a batch is built and captured once (``capture_all``) and then serves group after group of frames through
    ``reset(f, inputs, init_seed)``; a last group of fewer than B frames runs with ``active < B`` (the first ``active`` rows)."""

    def __init__(self, inputs, config, device, init_seeds=None, max_instances=None, max_views=None, max_label_views=None, photometric=False,
                 surface=False):
        """``max_instances`` and ``max_views`` None: every frame has ONE shape (views, height, width, instances).  ``max_instances`` an
        integer: a MIXED batch -- the frames have 1..max_instances instances each; every row is laid out for ``max_instances`` (the capacity)
        and carries its frame's own count in a header (include/vsrd_hip.h, vsrd_frame_header), and frame f still walks, bit for bit, the
        trajectory it walks in a slot of its own N, through both phases.  ``max_views`` an integer (1..32): likewise the frames have
        1..max_views views each and every row is laid out for ``max_views`` views (ABI 12).  The two combine; giving either one gives every
        row a header, and the axis without a capacity stays uniform.  The frames always share (height, width).  ``max_label_views``: the
        label-view capacity of every row (``group_labels``; the frames' groups may differ in size whatever the other capacities are, their
        count lives in the row) -- None: the largest L of the frames given, 0: no groups.
        ``photometric``: with a non-zero loss_weights["photometric_loss"], carry the photometric term in the batch -- every row gains the gray
        planes of its views ([view capacity, H, W] floats: 36 MB at 17 x 376 x 1408), the hard-mask weights of its target view with their
        ray table, and the workspace of vsrd_frame_photometric, and every residual step issues the batched draw,
        vsrd_frame_photometric_with_header and the batched finish (the term's field evaluations run the exact-fp32 MLP).  Every frame then
        needs its images and at least surface_top_k views.  The default refuses such a config; with weight 0 the keyword changes nothing.
        ``surface``: lay every row out for the buffers of ``surface()`` as well (whole images: 5.7 MB per row at 376 x 1408)."""
        inputs = list(inputs)
        self.surface_rows = bool(surface)
        if not inputs:
            raise ValueError("FrameBatch needs at least one frame")
        _check_loss_weights(config)
        self.photometric = bool(photometric) and photometric_weight(config) != 0.0
        if photometric_weight(config) != 0.0 and not photometric:
            raise ValueError("loss_weights['photometric_loss'] is non-zero: the photometric term is not batched over frames unless asked for "
                             "-- FrameBatch(..., photometric=True) gives every row the term's buffers (gray planes, hard-mask table, workspace); "
                             "or optimise such frames in FrameOptimizer loops")
        for position, frame_inputs in enumerate(inputs):        # (before any device work: a frame without images, or with fewer views than top_k)
            try:
                _check_photometric(frame_inputs, config, frame_inputs.soft_masks.shape[0], frame_inputs.soft_masks.shape[-1])
            except ValueError as error:
                raise ValueError(f"frame {position} of the batch: {error}") from None
        largest = max(label_view_count(i) for i in inputs)
        self.max_label_views = largest if max_label_views is None else int(max_label_views)
        if not 0 <= self.max_label_views <= _lib.MAX_LABEL_VIEWS:
            raise ValueError(f"max_label_views: 0..{_lib.MAX_LABEL_VIEWS}, got {self.max_label_views}")
        if largest > self.max_label_views > 0:
            raise ValueError(f"a frame with {largest} label views in a batch laid out for {self.max_label_views} (max_label_views)")
        shape = tuple(int(x) for x in inputs[0].soft_masks.shape)
        self.max_instances = None if max_instances is None else int(max_instances)
        self.max_views = None if max_views is None else int(max_views)
        if self.max_instances is None and self.max_views is None:
            if any(tuple(i.soft_masks.shape) != shape or tuple(i.image_size) != tuple(inputs[0].image_size) for i in inputs):
                raise ValueError("the frames of a batch share ONE shape (views, height, width, instances): frames that differ in instance or view "
                                 "count need max_instances / max_views")
        else:
            if self.max_instances is not None and not 1 <= self.max_instances <= _lib.MAX_INSTANCES:
                raise ValueError(f"max_instances: 1..{_lib.MAX_INSTANCES}, got {self.max_instances}")
            if self.max_views is not None and not 1 <= self.max_views <= _lib.MAX_VIEWS:
                raise ValueError(f"max_views: 1..{_lib.MAX_VIEWS}, got {self.max_views}")
            if any(tuple(i.soft_masks.shape[1:3]) != shape[1:3] or tuple(i.image_size) != tuple(inputs[0].image_size) for i in inputs):
                raise ValueError("the frames of a mixed batch share (height, width)")
            if self.max_views is None and any(int(i.soft_masks.shape[0]) != shape[0] for i in inputs):
                raise ValueError("the frames differ in view count: a batch of such frames needs max_views")
            if self.max_instances is None and any(int(i.soft_masks.shape[-1]) != shape[-1] for i in inputs):
                raise ValueError("the frames differ in instance count: a batch of such frames needs max_instances")
            if self.max_views is not None and any(not 1 <= int(i.soft_masks.shape[0]) <= self.max_views for i in inputs):
                raise ValueError(f"the frames of this batch have 1..max_views = {self.max_views} views")
            if self.max_instances is not None and any(not 1 <= int(i.soft_masks.shape[-1]) <= self.max_instances for i in inputs):
                raise ValueError(f"the frames of a mixed batch have 1..max_instances = {self.max_instances} instances")
            # (the rows' layout: both capacities; the axis without one is uniform, and its count is the capacity)
            shape = (shape[0] if self.max_views is None else self.max_views, *shape[1:3], shape[3] if self.max_instances is None else self.max_instances)
        capacities = (None, None) if self.max_instances is None and self.max_views is None else (shape[3], shape[0])
        self.size = len(inputs)
        import dataclasses
        if config.mlp_adjoint_item_slots == 0:
            config = dataclasses.replace(config, mlp_adjoint_item_slots=self.item_slots(self.size, config, shape[-1]))
        self.config, self.device = config, _indexed(device)
        with _capture_lock:
            self.arena = FrameArena(self.size, self._row_bytes(shape, config, self.max_label_views, headed=capacities != (None, None),
                                                               photometric=self.photometric, surface=self.surface_rows), self.device)
        # A row is FOUNDED on a frame that suits the table sampler its graphs will draw from (the frames a row later serves come through reset(),
        # which says so when one does not suit).  A founder that does not suit is replaced by the first one that does -- the shape is what a
        # row needs from its founder -- and listed in `unsuitable_founders`; no suitable founder at all: UnsuitableFrameError.
        self.frames, self.unsuitable_founders = [], []
        stand_in = None
        for f in range(self.size):
            cfg = config if init_seeds is None else dataclasses.replace(config, init_seed=init_seeds[f])
            row = self.arena.rows[f]
            candidates = [inputs[f]] + ([stand_in] if stand_in is not None else inputs[f + 1:])
            for position, frame_inputs in enumerate(candidates):
                row.cursor, row.layout = 0, []                           # (a founder that failed had begun to fill the row)
                try:
                    member = FrameOptimizer(frame_inputs, cfg, self.device, graph=True, persistent=True, row=row, capacity=capacities[0],
                                            view_capacity=capacities[1], max_label_views=self.max_label_views)
                except UnsuitableFrameError:
                    if position == 0:
                        self.unsuitable_founders.append(f)
                    if position + 1 == len(candidates):
                        raise
                    continue
                if stand_in is None:
                    stand_in = frame_inputs
                self.frames.append(member)
                break
        lead = self.arena.rows[0].layout
        for row in self.arena.rows[1:]:
            if row.layout != lead:
                raise RuntimeError("the frames of a batch laid their buffers out differently: frame batches need equal offsets in every row")
        self._graphs = {}
        self._eager_graph_steps = {}
        self._capture_stream = None

    @staticmethod
    def item_slots(num_frames, config, num_instances):
        """Slots per work item of the MLP adjoint for a batch of `num_frames` frames (vsrd_render_config::adjoint_slots_per_item): the library
        plans about 16384 items per LAUNCH from one frame's size; a batch has B times the items, so its items can be B times as large --
        fewer partial rows to write and to sum (measured, 1000 rays x 100 samples, N = 8: 8 frames 0.392 -> 0.337 ms per frame-step with 16
        slots, 4 frames 0.423 -> 0.379; profiles/r06_native).  The next power of two, 4..32."""
        rounds = 2 if config.num_samples <= 64 else 4
        wanted = num_frames * config.num_rays * rounds * num_instances / 16384.0
        slots = 4
        while slots < wanted and slots < 32:
            slots *= 2
        return slots

    @staticmethod
    def _row_bytes(shape, config, label_views=0, headed=False, photometric=False, surface=False):
        """Bytes of one frame's row: the aligned sizes of everything a FrameOptimizer(row=...) creates there, summed over the declarations it
        allocates from and the regions the library sizes, in the order of allocation (Adam's state, declared with the parameters, comes
        amid the glue) -- every output included, so a row is exactly full once each has been asked for.  `headed`: rows with a header;
        `photometric`: rows that carry the photometric term (nothing is added while its weight is 0); `surface`: rows that hold the
        buffers of surface().  Which rows hold which output: _FrameOutput.held, over these switches."""
        V, H, W, N = (int(x) for x in shape)
        def sizes(declared):
            return [_buffer_bytes(shape, dtype) for _, shape, dtype, _ in declared]
        parts = sizes(_parameter_buffers(N) + _scalar_buffers(config))
        parts += [rendering.Workspace.adjoint_bytes(N, True, (config.num_samples, config.num_rays))]
        parts += sizes(_ray_buffers(V, N, H, W)) + [_lib.load().vsrd_ray_table_bytes(V * H * W)]
        parts += sizes(_glue_buffers(V, N, config, headed))
        if config.scalar_interval > 0 or config.checkpoint_interval > 0:
            parts += sizes(_log_buffers(N, config))
        if photometric and photometric_weight(config) != 0.0:
            parts += sizes(_photometric_buffers(V, N, H, W, config)) + [_lib.load().vsrd_ray_table_bytes(H * W)]
        switches = dict(label_views=int(label_views), headed=headed, photometric=photometric, surface=surface)
        leading = dict(view_capacity=V, label_view_capacity=int(label_views))
        for output in _OUTPUTS.values():
            if output.held(switches):
                parts += sizes(output.buffers(leading[output.leading], N, H, W))
        return sum(FrameArena.aligned(nbytes) for nbytes in parts)

    # ---- one step of the first `active` frames -----------------------------------------------------------------------------------
    def _members(self, active):
        active = self.size if active is None else int(active)
        if not 1 <= active <= self.size:
            raise ValueError(f"active frames: 1..{self.size}, got {active}")
        return active, self.frames[:active]

    def _step(self, active, count=True, joins=(True, True)):
        active, members = self._members(active)
        lead = members[0]
        if any(m.step_index != lead.step_index for m in members):
            raise RuntimeError("the frames of a batch step together: reset() every active frame before running the batch")
        with rendering.workspace_scope(lead.workspace):
            if not torch.cuda.is_current_stream_capturing():
                for m in members:
                    m._check_bindings()
            lead._fused_step(None, count=False, joins=joins, frames=(active, self.arena.stride))
        if count:
            for m in members:
                m.step_index += 1

    def outputs(self, f):
        """Frame f's record of its last step: the dictionary ``FrameOptimizer.step`` returns (device tensors, rewritten by every step)."""
        m = self.frames[f]
        # (step_index counts the steps done: the last one had index step_index - 1, and `step_index - 1 >= warmup_steps` is its `residual`)
        return m._step_record(m.step_index > self.config.warmup_steps)

    def _ask(self, name, active, inputs=(), **arguments):
        """Output `name` (_OUTPUTS) of the first ``active`` frames: first use creates its buffers in EVERY row, so that the rows keep equal
        offsets, and every active frame takes the call's own `inputs` (one dictionary each: _FrameOutput.take); then ONE launch on row 0
        covers the first ``active`` rows, and every frame gets its own views."""
        active, members = self._members(active)
        _check_asked(name, members)
        for m in self.frames:
            m._output_state(name)
        for m, own in zip(members, inputs):
            m._take(name, own)
        if any(row.layout != self.arena.rows[0].layout for row in self.arena.rows[1:]):
            raise RuntimeError(f"the frames of a batch laid their {name} buffers out differently: frame batches need equal offsets in every row")
        self.frames[0]._launch_output(name, frames=(active, self.arena.stride), **arguments)
        return [_OUTPUTS[name].views(m, m._outputs[name], **arguments) for m in members]

    def labels(self, active=None):
        """The pseudo-labels of the first ``active`` frames (``FrameOptimizer.labels``) by ONE vsrd_frame_labels call for all of them: a
        list of dictionaries of device tensors, each sliced to its frame's own instance count."""
        return self._ask("labels", active)

    def group_labels(self, active=None):
        """The pseudo-labels of the first ``active`` frames in the views of their groups (``FrameOptimizer.group_labels``) by ONE
        vsrd_frame_group_labels call for all of them, whatever their groups' sizes: a list of dictionaries of device tensors, each sliced to
        its frame's own label views and instances.  ValueError when an active frame has no group."""
        for m in self._members(active)[1]:
            m._check_has_group()
        return self._ask("group_labels", active)

    def masks(self, active=None, view=0, threshold=0.5, soft=False):
        """The dense predicted masks of the first ``active`` frames (``FrameOptimizer.masks``) by ONE vsrd_frame_masks call for all of
        them: a list of dictionaries of device tensors, each sliced to its frame's own instance count.  ``view`` must exist in every
        active frame."""
        _check_view(view, self._members(active)[1])
        return self._ask("masks", active, view=view, threshold=threshold, soft=soft)

    def surface(self, active=None, view=0, hard=True, light=None, shadows=True, background=None, alpha=None):
        """The dense surface renders of the first ``active`` frames (``FrameOptimizer.surface``) by ONE vsrd_frame_surface call for all of
        them: a list of dictionaries of device tensors.  ``view`` must exist in every active frame; ``background``: None, or one
        [H,W,3] uint8 image per active frame.  The batch must have been built with ``surface=True`` (its rows hold the images)."""
        if not self.surface_rows:
            raise RuntimeError("surface(): this batch's rows were laid out without the surface buffers -- FrameBatch(..., surface=True)")
        active, members = self._members(active)
        _check_view(view, members)
        if background is not None and len(background) != active:
            raise ValueError(f"background: one image per active frame ({active}), got {len(background)}")
        inputs = [dict(light=light, background=None if background is None else background[k]) for k in range(active)]
        return self._ask("surface", active, inputs, view=view, hard=hard, shadows=shadows, background=background is not None, alpha=alpha)

    def metrics(self, active=None):
        """The 3-D / BEV IoU metrics of the first ``active`` frames (``FrameOptimizer.metrics``) by ONE vsrd_frame_metrics call for all of
        them: a list of dictionaries of device tensors, each sliced to its frame's own instance count.  A frame without ``boxes_3d`` is not
        an error here: its IoUs are NaN and its summary is eight zeros (count 0), for which ``formats.frame_metrics`` gives {}."""
        return self._ask("metrics", active)

    def _phase(self, active):
        _, members = self._members(active)
        return members[0].step_index >= self.config.warmup_steps

    def step(self, active=None):
        """One optimisation step of the first ``active`` frames: three eager steps per (phase, active) warm the lazy initialisations, then the
        step is captured once and replayed (``_advance``)."""
        self._graph_advance(1, active)

    def _graph_advance(self, k, active=None):
        """``k`` steps of the first ``active`` frames (``_advance``) under the batch's key (phase, active, k), then the members' step counts
        and the log launch that follows a step group when one of them sits on a boundary."""
        active, members = self._members(active)
        _advance(self, (self._phase(active), active, k), k, lambda _, **how: self._step(active, **how))
        for m in members:
            m.step_index += k
        _launch_log(members, frames=(active, self.arena.stride))

    def log_outputs(self, metrics=False, masks=False):
        """``FrameOptimizer.log_outputs`` for every row (the outputs' buffers at equal offsets)."""
        for m in self.frames:
            m.log_outputs(metrics=metrics, masks=masks)
        if any(row.layout != self.arena.rows[0].layout for row in self.arena.rows[1:]):
            raise RuntimeError("the frames of a batch laid their output buffers out differently: frame batches need equal offsets in every row")

    def history(self, active=None):
        """``FrameOptimizer.history`` of the first ``active`` frames: a list of dictionaries of device tensors, each sliced to its frame's own rows."""
        return [m.history() for m in self._members(active)[1]]

    def snapshots(self, active=None):
        """``FrameOptimizer.snapshots`` of the first ``active`` frames: a list of lists, each frame's own slots and instances."""
        return [m.snapshots() for m in self._members(active)[1]]

    def run(self, num_steps, steps_per_graph=4, active=None):
        """``num_steps`` steps of the first ``active`` frames; whole groups of ``steps_per_graph`` steps inside a phase replay ONE hipGraph."""
        active, members = self._members(active)
        remaining = int(num_steps)
        while remaining > 0:
            residual = self._phase(active)
            # (no group crosses a boundary of the log, of any row)
            k = _steps_in_next_group(remaining, None if residual else self.config.warmup_steps - members[0].step_index, _steps_to_log_boundary(members),
                                     steps_per_graph, (residual, active, 1) in self._graphs)
            self._graph_advance(k, active)
            remaining -= k

    def capture_all(self, steps_per_graph=4, actives=None):
        """Every eager warm-up step and every capture ``run()`` would meet -- both phases, the one-step and the ``steps_per_graph``-step graph,
        for every frame count in ``actives`` (default: the full batch) -- now, then every frame is reset.  Returns the number of graphs."""
        k = int(steps_per_graph)
        for active in (actives or [self.size]):
            _capture_phases(self._members(active)[1], k, lambda: self.step(active), lambda: self._graph_advance(k, active))
        with _capture_lock:
            torch.cuda.current_stream(self.device).synchronize()
        for m in self.frames:
            m.reset(m.inputs)
        return len(self._graphs)

    def reset(self, f, inputs, init_seed=None):
        """Row f starts another frame (``FrameOptimizer.reset``; a mixed batch's row takes any frame of its image size with 1..max_instances
        instances and 1..max_views views -- the rows' capacities -- ValueError otherwise).  False: the frame does not suit the table sampler -- optimise it in a loop of its own."""
        return self.frames[f].reset(inputs, init_seed=init_seed)

    def close(self):
        _destroy_graphs(self._graphs)
        for m in self.frames:
            m.close()

    def __del__(self):
        try:
            _destroy_graphs(self._graphs, wait=False)
        except Exception:
            pass
