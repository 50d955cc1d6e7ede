"""Frame-sharded multi-GPU launcher: one rank process per GPU on RCCL (the default since round 6: a rank optimises `--frame-batch` frames in
lock-step, optimization.FrameBatch, which fills the GPU from ONE process; `--procs-per-gpu P` > 1 -- round 5's answer, P processes per GPU
with a gloo control plane -- is still there), frames handed to the ranks from a shared queue (or split statically), no data-path collective;
persistent frame slots / batches inside a rank; a supervisor that restarts dead ranks.

Reference behaviour (scripts/main.py:45-57, vsrd/distributed/loader.py:4-9, README.md:128): ``torch.distributed`` is
initialised, ranks print in order between barriers, a ``DistributedSampler`` hands every rank its share of the target
frames, and each rank optimises its frames alone -- gradients are never averaged.  The only traffic is the start-up
barrier; here additionally rank 0 broadcasts the run manifest so every rank agrees on the frame list.  On ROCm the
``nccl`` backend is RCCL (xGMI carries latency-only messages; nothing bandwidth-bound exists on this path).
"""
import os
import random
import re
from typing import Callable, List, Sequence

import torch
import torch.distributed as dist


def init_process_group(backend=None, ranks_per_device=1):
    """env:// rendezvous as with torchrun (main.py:49).  Returns (rank, world_size, device).  `ranks_per_device` consecutive local ranks
    share a device (the launcher's --procs-per-gpu)."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0")) // max(int(ranks_per_device), 1)
    use_gpu = torch.cuda.is_available()
    device = torch.device("cuda", local % max(torch.cuda.device_count(), 1)) if use_gpu else torch.device("cpu")
    if use_gpu:
        torch.cuda.set_device(device)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend=backend or ("nccl" if use_gpu else "gloo"), rank=rank, world_size=world)
    return rank, world, device


def barrier():
    if dist.is_available() and dist.is_initialized():
        if dist.get_backend() == "gloo":
            # (dist.barrier() asks the HIP runtime for devices before it settles on gloo's host barrier: on a GPU node that opens the
            #  device in every rank, the GPU-free selftest ranks included.  A one-element host all_reduce is the same barrier without it.)
            dist.all_reduce(torch.zeros(1))
        else:
            dist.barrier()


def ordered(action: Callable[[int], None]):
    """Run ``action(rank)`` rank by rank between barriers (the ordered start-up print of main.py:53-57)."""
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    for turn in range(world):
        if turn == rank:
            action(rank)
        barrier()


def broadcast_manifest(manifest=None):
    """Rank 0's manifest (any picklable object) to every rank."""
    if not (dist.is_available() and dist.is_initialized()):
        return manifest
    box = [manifest if dist.get_rank() == 0 else None]
    dist.broadcast_object_list(box, src=0)
    return box[0]


def shard_frames(frames: Sequence, rank: int, world_size: int, seed: int = 0) -> List:
    """Seeded permutation, then frame j of the permutation goes to rank j mod world_size.

    Unlike ``DistributedSampler`` (loader.py:8) no frame is duplicated to pad the shards: the reference relies on its
    "skip if the final checkpoint exists" guard (main.py:134-136) to make the padded duplicates harmless; here they never exist.
    """
    order = list(range(len(frames)))
    random.Random(seed).shuffle(order)
    return [frames[j] for position, j in enumerate(order) if position % world_size == rank]


class FrameQueue:
    """Where a rank's next frames come from.

    ``static``: the rank's own shard (``shard_frames``: frame j of the seeded permutation to rank j mod world), fixed before the clock starts.
    ``dynamic`` (SURVEY section 8e "tail imbalance"): ONE queue for the job -- the seeded permutation of the manifest's
    frames -- and a rank that has nothing left to do takes the next ``n`` frames of it with one atomic ``TCPStore.add`` on a counter that rank 0's
    store serves.  No collective, nobody waits for anybody: real frames differ in instance count and cost, and with a static split the job
    ends when the unluckiest rank does; with the queue the ranks finish within one group of frames of each other.  The skip-if-done guard
    (main.py:134-136) makes a restarted job idempotent either way: the queue of a new attempt starts over and finished frames are skipped."""

    def __init__(self, frames, rank=0, world=1, seed=0, store=None, key="vsrd_next_frame"):
        self.dynamic = store is not None
        self.store, self.key = store, key
        order = list(range(len(frames)))
        random.Random(seed).shuffle(order)
        self.order = [frames[j] for j in order]
        self.mine = [f for position, f in enumerate(self.order) if position % world == rank]       # (= shard_frames: the static split)
        self.cursor = 0
        self.taken = []

    def take(self, n=1):
        """The next (at most) ``n`` frames for this rank; [] when the job has none left."""
        n = max(int(n), 1)
        if self.dynamic:
            end = int(self.store.add(self.key, n))
            group = self.order[max(end - n, 0):min(end, len(self.order))] if end - n < len(self.order) else []
        else:
            group = self.mine[self.cursor:self.cursor + n]
            self.cursor += len(group)
        self.taken += group
        return group


def pending_frames(frames: Sequence, checkpoint_path: Callable[[object], str] = None):
    """[(frame, path)] of the frames whose final checkpoint does not exist yet (main.py:134-136), with what a rank that was killed inside
    formats.atomic_torch_save left behind in their folders removed (the frame is this rank's now: nobody else writes there)."""
    pending = []
    for frame in frames:
        path = checkpoint_path(frame) if checkpoint_path else None
        if not (path and os.path.exists(path)):
            pending.append((frame, path))
            folder, stem = (os.path.dirname(path), os.path.basename(path) + ".tmp.") if path else (None, None)
            if folder and os.path.isdir(folder):
                for name in os.listdir(folder):
                    if name.startswith(stem):
                        os.remove(os.path.join(folder, name))
    return pending


def run_frames(frames, optimise: Callable, checkpoint_path: Callable[[object], str] = None, frames_in_flight: int = 1, save: Callable = None):
    """Optimise this rank's frames -- a sequence, or a ``FrameQueue`` the frames are taken from one by one -- skipping every frame whose final
    checkpoint exists (main.py:134-136).

    ``frames_in_flight`` > 1 runs that many frames at the same time on this rank's GPU, one host thread and one stream each: at the
    reference's 1000 rays per step the launch-bound box-only phase runs twice as fast with two frames, the compute-bound residual
    phase about 10 % faster.  ``optimise`` is then called from worker threads, inside ``torch.cuda.stream(<own stream>)``; a
    ``FrameOptimizer(graph=True)`` built there is safe because nothing it calls into HIP -- construction, eager warm-up steps, replay
    launches, graph destruction, host synchronisations -- runs during ANOTHER frame's capture, and captures (with a graph's first launch)
    run alone: optimization._CaptureGate (round 4, one box: 0.749 frames/s with one frame in flight, 0.91 with three; without the gate a
    dead rank about every tenth run of 36 frames).
    ``save(result, path)`` writes a frame's final checkpoint (default: formats.atomic_torch_save).
    Returns the frames optimised, in the order of ``frames`` (a queue: in the order they were taken)."""
    import threading

    def source():
        if hasattr(frames, "take"):
            while True:
                group = frames.take(1)
                if not group:
                    return
                yield group[0]
        else:
            yield from frames

    numbered = enumerate(source())
    take_lock = threading.Lock()

    def next_pending():
        """(index, frame, path) of the next frame that still has to be optimised, or None."""
        while True:
            with take_lock:
                item = next(numbered, None)
            if item is None:
                return None
            found = pending_frames([item[1]], checkpoint_path)
            if found:
                return item[0], found[0][0], found[0][1]

    def work():
        finished = []
        while True:
            item = next_pending()
            if item is None:
                return finished
            index, frame, path = item
            result = optimise(frame)
            if path:
                from .formats import atomic_torch_save
                (save or atomic_torch_save)(result, path)   # utils.Saver.save == torch.save(dict) (vsrd/utils.py:191-198), written atomically
            finished.append((index, frame))

    if frames_in_flight <= 1:
        return [frame for _, frame in work()]

    from concurrent.futures import ThreadPoolExecutor
    # a worker thread starts with device 0 current: it takes over this thread's device (the rank's GPU) before it makes its stream
    device = torch.cuda.current_device() if torch.cuda.is_available() else None

    def on_own_stream():
        if torch.cuda.is_available():
            torch.cuda.set_device(device)
            from . import optimization
            with torch.cuda.stream(torch.cuda.Stream(device=device)):
                finished = work()
                with optimization.exclusive_device_access():      # (a host synchronisation: not next to another frame's capture)
                    torch.cuda.current_stream().synchronize()
                return finished
        return work()

    with ThreadPoolExecutor(max_workers=frames_in_flight) as pool:
        futures = [pool.submit(on_own_stream) for _ in range(frames_in_flight)]
        finished = [item for future in futures for item in future.result()]
    return [frame for _, frame in sorted(finished, key=lambda item: item[0])]


# ---------------------------------------------------------------------------------------------------------------------------------
# frames/s: the unit the reference shards (README.md:128 "about 15 minutes per frame"; main.py:106-136 one optimisation per frame)
#   python -m vsrd_amd.launcher --gpus N --frames K      (or under torchrun; `python bench.py --native --gpus N ...` forwards here)
# ---------------------------------------------------------------------------------------------------------------------------------

def synthetic_frame_inputs(device, frame, views, instances, height=376, width=1408, label_views=0, images=False):
    """FrameInputs of synthetic frame number `frame` (synthetic.synthetic_frame(seed = frame): KITTI-360 intrinsics, boxes in the
    reference's ranges): soft masks rendered from the true boxes at the sharp end of the schedule, ground-truth 2-D boxes projected
    from them, every instance visible in every view; the true boxes' corners are the frame's 3-D ground truth (boxes_3d).
    ``label_views`` L > 0: the frame also carries a group of L label views (synthetic.synthetic_group).  ``images``: it carries the views'
    colour images (synthetic.synthetic_images, x / 255), which the photometric term needs."""
    from . import fields, models, operations, optimization, rendering, synthetic
    K, E, raw_loc, raw_dim, raw_ori = synthetic.synthetic_frame(int(frame), views, height, width, instances)
    K, E = K.to(device), E.to(device)
    det = models.BoxParameters3D(1, instances).to(device)
    with torch.no_grad():
        det.locations.copy_(raw_loc); det.dimensions.copy_(raw_dim); det.orientations.copy_(raw_ori)
        out = det()
        cam, dirs = rendering.ray_casting((height, width), K, E)
        block = fields.FieldBlock(fields.pack_instances(out["locations"][0], out["orientations"][0], out["dimensions"][0]), 0.1, None, None)
        origins = cam[:, None, None, :].expand(views, height, width, 3).reshape(-1, 3).contiguous()
        soft = rendering.render_hierarchical(block, origins, dirs.reshape(-1, 3), (0.0, 100.0), 64, 0.1, 1.0, seed=1,
                                             skip_exact_misses=True)["labels"].clamp(0, 1).reshape(views, height, width, instances).contiguous()
        gt_boxes, _ = operations.project_boxes_multi_view(out["boxes_3d"][0], E, K, (height, width))
    group = {key: value.to(device) for key, value in synthetic.synthetic_group(frame, height, width, label_views, out["boxes_3d"][0].cpu()).items()} \
        if label_views else {}
    return optimization.FrameInputs((height, width), K, E, soft, gt_boxes, torch.ones(views, instances, dtype=torch.bool, device=device),
                                    boxes_3d=out["boxes_3d"][0].contiguous(), **group,
                                    images=synthetic.synthetic_images(frame, views, height, width).to(device).to(torch.float32) / 255.0 if images else None)


def scan_frames_dir(folder, limit=0):
    """--frames-dir: the sorted *.npz files of `folder` (the first `limit` of them when limit > 0) and each one's
    (V, H, W, N) (frames.pack_counts: no masks are loaded).  The packs of one job share their image size; their view and instance
    counts may differ (1..32 views, 1..64 instances: the batch rows' capacities are the maxima over the job).  SystemExit when there is no
    pack, when a file is malformed, has a count outside those limits, or an (H, W) that differs from the first one's -- naming the odd file."""
    import glob
    from . import frames
    files = sorted(glob.glob(os.path.join(folder, "*.npz")))
    if not files:
        raise SystemExit(f"--frames-dir {folder}: no *.npz frame packs there")
    if limit > 0:
        if limit > len(files):
            raise SystemExit(f"--frames {limit}: --frames-dir {folder} holds {len(files)} frame packs")
        files = files[:limit]
    shapes = []
    for path in files:
        try:
            shapes.append(frames.pack_counts(path))
        except ValueError as error:
            raise SystemExit(f"--frames-dir: {error}")
        if shapes[-1][1:3] != shapes[0][1:3]:
            raise SystemExit(f"--frames-dir: {path} has (height, width) = {shapes[-1][1:3]}, {files[0]} has {shapes[0][1:3]}: "
                             "the frames of one job share their image size")
        if not 1 <= shapes[-1][0] <= 32:
            raise SystemExit(f"--frames-dir: {path} has {shapes[-1][0]} views, 1..32")
        if not 1 <= shapes[-1][3] <= 64:
            raise SystemExit(f"--frames-dir: {path} has {shapes[-1][3]} target instances, 1..64")
    return files, shapes


def scan_label_views(files):
    """--group-predictions with --frames-dir: every pack's L (frames.pack_label_views: nothing else is read); the rows' label-view capacity
    is the job's largest.  SystemExit naming the first pack that carries no group."""
    from . import frames
    counts = []
    for path in files:
        try:
            counts.append(frames.pack_label_views(path))
        except ValueError as error:
            raise SystemExit(f"--frames-dir: {error}")
        if counts[-1] < 1:
            raise SystemExit(f"--group-predictions: {path} carries no group (label_frame_ids, label_intrinsic_matrices, label_extrinsic_matrices, "
                             "label_boxes_2d, label_visible): the exporter writes them from the dataset's grouped frames")
        if counts[-1] > frames.MAX_LABEL_VIEWS:
            raise SystemExit(f"--frames-dir: {path} has {counts[-1]} label views, 1..{frames.MAX_LABEL_VIEWS}")
    return counts


def parse_light(text):
    """--surface-light "X,Y,Z" -> (x, y, z), None for the empty string (the default light); ValueError for anything that is not three finite
    numbers with a direction (not all zero)."""
    if not text:
        return None
    import math
    try:
        light = tuple(float(part) for part in text.split(","))
    except ValueError:
        light = ()
    if len(light) != 3 or not all(math.isfinite(x) for x in light) or not any(light):
        raise ValueError(f"--surface-light: three finite numbers X,Y,Z, not all zero, got {text!r}")
    return light


def scan_images(files):
    """--photometric with --frames-dir: every pack must carry the views' images (frames.FramePack.images); the first one without is named."""
    from . import frames
    for path in files:
        try:
            present = frames.pack_has_images(path)
        except ValueError as error:
            raise SystemExit(f"--frames-dir: {error}")
        if not present:
            raise SystemExit(f"--photometric: the frame pack {path} carries no images (the optional member `images`, [V,3,H,W] uint8: "
                             "tools/make_frame_packs.py --images writes it)")


def _newest_change(folder):
    """Modification time of the newest entry of the checkpoint directory: a frame's folder changes when its checkpoint is renamed into it."""
    try:
        return max([os.stat(folder).st_mtime, *(entry.stat().st_mtime for entry in os.scandir(folder))])      # (the folder itself: rank 0 touches it when its set-up is done)
    except OSError:
        return 0.0


def _wait_for_ranks(children, grace_seconds=10.0, progress_folder=None, stall_seconds=0.0):
    """Poll the ranks until all have exited.  The first rank that exits non-zero takes the others with it (SIGTERM, SIGKILL after
    `grace_seconds`): a rank whose peer died would otherwise sit in its final barrier until the collective's watchdog fires, tens of
    minutes later.  `stall_seconds` > 0: an attempt during which NO checkpoint appears in `progress_folder` for that long (counted from the
    attempt's start) ends the same way -- a rank that hangs inside the runtime exits with nothing, and its peers wait for it for ever.
    Returns None when every rank exited 0, else (rank, exit code) of the first failure ((-1, 124) for a stall)."""
    import time
    pending = dict(enumerate(children))
    failed, deadline = None, None
    started = time.time()
    while pending:
        for rank, child in list(pending.items()):
            code = child.poll()
            if code is None:
                continue
            del pending[rank]
            if code != 0 and failed is None:
                failed, deadline = (rank, code), time.monotonic() + grace_seconds
                for other in pending.values():
                    other.terminate()
        if failed is None and pending and stall_seconds > 0 and time.time() - max(started, _newest_change(progress_folder)) > stall_seconds:
            failed, deadline = (-1, 124), time.monotonic() + grace_seconds
            for other in pending.values():
                other.terminate()
        if failed is not None and pending and time.monotonic() > deadline:
            for other in pending.values():
                other.kill()
            deadline = float("inf")
        if pending:
            time.sleep(0.05)
    return failed


def _supervise(argv, args):
    """No launcher around us: this process stays GPU-free and supervises `--gpus` rank processes (README.md:146-155: the reference leans on
    `torchrun --max_restarts` for the same thing, and on its skip-if-done guard, main.py:134-136, for what a restart repeats).

    A rank that dies -- a segmentation fault inside the runtime, an out-of-memory kill -- strands its shard and leaves its peers in a
    barrier.  The supervisor ends the attempt (see _wait_for_ranks) and starts ALL ranks again as FRESH child processes, up to
    `--max-restarts` times: nothing that has initialised a GPU is ever re-executed, the rendezvous gets a new port, and every frame whose
    final checkpoint exists is skipped, so a restart costs the frames that were in flight.  The checkpoint directory therefore has to
    outlive an attempt: the supervisor fixes it (a temporary directory unless --out names one) and hands it to the ranks."""
    import socket
    import subprocess
    import sys
    import tempfile
    # (counting devices does not initialise the runtime on this image; a selftest has no devices to count)
    if not args.ranks_share_gpu and not args.selftest and torch.cuda.device_count() < args.gpus:
        raise SystemExit(f"vsrd_amd.launcher --gpus {args.gpus}: this node has {torch.cuda.device_count()} visible GPU(s)")
    ranks = args.gpus * args.procs_per_gpu
    out_dir = args.out or tempfile.mkdtemp(prefix="vsrd_frames_")
    if not args.out:
        argv = list(argv) + ["--out", out_dir]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    failed = None
    for attempt in range(args.max_restarts + 1):
        with socket.socket() as s:                 # (a free port now; should somebody take it before rank 0 binds it, the attempt fails and the next one asks again)
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        children = []
        for rank in range(ranks):
            env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(ranks), LOCAL_WORLD_SIZE=str(ranks), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            children.append(subprocess.Popen([sys.executable, "-m", "vsrd_amd.launcher", *argv, "--attempt", str(attempt)], env=env, cwd=root))
        failed = _wait_for_ranks(children, progress_folder=out_dir, stall_seconds=args.stall_timeout)
        if failed is None:
            if not args.out:                   # (the supervisor's own temporary directory -- full per-frame checkpoints -- goes with the job)
                import shutil
                shutil.rmtree(out_dir, ignore_errors=True)
            return 0
        again = attempt < args.max_restarts
        print(f"[vsrd_amd.launcher] attempt {attempt}: " + (f"no checkpoint for {args.stall_timeout:g} s (--stall-timeout): the ranks were ended; " if failed[0] < 0 else
                                                           f"rank {failed[0]} exited with code {failed[1]}; ")
              + ("starting the ranks again as fresh processes (frames with a final checkpoint are skipped)" if again else "no restarts left"),
              file=sys.stderr, flush=True)
    return abs(failed[1]) or 1


# ---- what the flags ask of a group of finished frames, in the order of asking: ONE list for the clock's keys (_RenderWork._begin_outputs) and
# for the collection (_RenderWork._collect).  `each(work, pending, frame, folder, entry, payload)`: what one frame's entry adds to the pending
# file writes and to its payload; `how(work, source, frames, active)`: the keyword arguments to ask with (None: this source is not asked)
def _to_file(key, save):
    from . import formats
    return lambda work, pending, frame, folder, entry, payload: pending.append((key, getattr(formats, save), (folder, formats.to_host(entry))))


def _masks_to_file(work, pending, frame, folder, entry, payload):
    from . import formats
    host = formats.to_host({key: value for key, value in entry.items() if key != "soft"})
    payload["metrics"] = dict(payload.get("metrics") or {}, mask_iou=float(host["mask_iou"].mean()))
    pending.append(("masks_write", formats.save_frame_masks, (folder, host, host["shape"])))


def _metrics_to_report(work, pending, frame, folder, entry, payload):
    from . import formats
    named = formats.frame_metrics(entry["summary"])
    if named:
        payload["metrics"] = dict(payload.get("metrics") or {}, **named)
        work.frame_metrics[int(frame)] = named


def _with_light(work, source, frames, active):      # (--surface: laid over the frames' photographs when every frame of the group carries one)
    photographs = [work.backgrounds.pop(int(frame), None) for frame, _ in frames]
    return dict(light=work.surface_light, background=photographs[0] if active is None else (photographs if all(p is not None for p in photographs) else None))


_plainly = lambda work, source, frames, active: {}
_OUTPUTS = [        # (flag, method of a FrameOptimizer / a FrameBatch, the clock's keys, each, how)
    ("predictions", "labels", ("labels", "labels_write"), _to_file("labels_write", "save_frame_labels"), _plainly),
    ("group_predictions", "group_labels", ("group_labels", "group_labels_write"), _to_file("group_labels_write", "save_frame_group_labels"), _plainly),
    ("masks", "masks", ("masks", "masks_write"), _masks_to_file, _plainly),
    ("surface", "surface", ("surface", "surface_write"), _to_file("surface_write", "save_frame_surface"), _with_light),
    # (a loop without 3-D ground truth is not asked; a batch is, and its frames without come back with count 0 and are skipped)
    ("metrics", "metrics", ("metrics",), _metrics_to_report, lambda work, source, frames, active: {} if active is not None or source.inputs.boxes_3d is not None else None)]


class _RenderWork:
    """What ONE PROCESS does with the frames it takes from the queue on its GPU: frame slots / the frame batch (and, with a static queue,
    the inputs) before the clock, then the frames."""

    def __init__(self, args, manifest, device, queue):
        self.args, self.manifest, self.device, self.queue = args, manifest, device, queue
        self.config = dict(num_steps=args.num_steps, warmup_steps=args.warmup_steps, num_rays=args.rays, num_samples=args.samples,
                           mlp_split_bf16=not args.fp32_mlp, mlp_adjoint_item_slots=args.adjoint_item_slots)
        # --scalar-interval / --ckpt-interval / --select: the device-side log of every frame (optimization.FrameOptimizer.history / snapshots)
        self.scalar_interval, self.ckpt_interval = int(getattr(args, "scalar_interval", 0) or 0), int(getattr(args, "ckpt_interval", 0) or 0)
        self.select = parse_select(getattr(args, "select", "") or "")
        self.logs = self.scalar_interval > 0 or self.ckpt_interval > 0
        if self.logs:
            self.config.update(scalar_interval=self.scalar_interval, checkpoint_interval=self.ckpt_interval)
        # --photometric W: the photometric term in every loop and every batch row of the job (FrameBatch(..., photometric=True))
        self.photometric = float(getattr(args, "photometric", 0.0) or 0.0)
        self.photometric_losses = {}
        self.backgrounds = {}            # --surface: frame -> uint8 [H,W,3] (_note_background)
        self.wanted = {flag: bool(getattr(args, flag, False)) for flag, *_ in _OUTPUTS}      # (the output flags, read HERE only: bare arguments may lack the newer ones)
        self.surface_light = getattr(args, "surface_light", None)
        if self.photometric:
            from . import losses
            self.config.update(loss_weights={**losses.LOSS_WEIGHTS, "photometric_loss": self.photometric})

    def path_of(self, frame):
        return os.path.join(self.manifest["out"], f"frame_{int(frame):06d}", f"step_{self.args.num_steps - 1}.pt")

    def init_seed(self, frame):
        # a frame starts from parameters drawn for (seed, frame): the same optimisation whichever rank, process, slot or batch row runs it
        # (the reference seeds once per rank, scripts/main.py:67-74)
        return (int(self.manifest["seed"]) * 1000003 + int(frame)) & 0x7FFFFFFF

    def inputs_of(self, frame):
        """A static queue's synthetic inputs are resident before the clock (what main.py:106-316 prepares per frame is the dataset's work, not the
        loop's); a dynamic queue's are built when the frame is taken -- inside the clock, like the reference's loader -- and dropped after.
        Frame packs (--frames-dir) are always read when the frame is taken and never kept."""
        if frame in self.inputs:
            return self._note_background(frame, self.inputs[frame])
        args = self.args
        if args.frames_dir:          # a frame pack (frames.py), host side: slots and batch rows reset from it, vsrd_frame_ingest fills the row
            from . import frames
            return self._note_background(frame, frames.load_pack(self.manifest["packs"][int(frame)]))
        return self._note_background(frame, synthetic_frame_inputs(self.device, frame, views_of(frame, args.view_counts), instances_of(frame, args.instance_counts),
                                                                   args.height, args.width, args.label_views, images=bool(self.photometric)))

    def _note_background(self, frame, inputs):
        """--surface: the target view's photograph of a frame that carries its images (a pack's member `images`, FrameInputs.images), as the
        uint8 [H,W,3] image the surface render is laid over -- kept from the moment the frame is taken until its outputs are collected."""
        images = getattr(inputs, "images", None)
        if self.wanted["surface"] and images is not None:
            first = torch.as_tensor(images[0])
            if first.dtype != torch.uint8:
                first = (first.to(torch.float32) * 255.0 + 0.5).clamp(0.0, 255.0).to(torch.uint8)
            self.backgrounds[int(frame)] = first.permute(1, 2, 0).contiguous()
        return inputs

    def materialised(self, inputs):
        """`inputs` as a FrameInputs on the device: what founds a slot or a batch, and what a loop of its own is built on."""
        from . import frames
        return frames.ingest(inputs, self.device) if isinstance(inputs, frames.FramePack) else inputs

    @staticmethod
    def count_of(inputs):
        from . import frames
        return inputs.num_instances if isinstance(inputs, frames.FramePack) else int(inputs.soft_masks.shape[-1])

    @staticmethod
    def views_of(inputs):
        from . import frames
        return inputs.num_views if isinstance(inputs, frames.FramePack) else int(inputs.soft_masks.shape[0])

    def optimization_config(self, **more):
        from . import optimization
        return optimization.OptimizationConfig(seed=int(self.manifest["seed"]), **self.config, **more)

    def prepare(self):
        """Before the clock: the frame slots (round 5) or the frame batch (round 6) -- every persistent loop constructed and ALL its hipGraphs
        captured here, before any worker thread exists -- and, with a static queue, this rank's inputs.  A frame is then a reset (copies and
        fills), graph replays and a checkpoint: no construction, no eager steps, no capture.  (--fresh-loops: the round-4 form, for A/B.)"""
        import queue
        import time
        from . import optimization
        args = self.args
        mine = [] if self.queue.dynamic else [frame for frame in self.queue.mine if not os.path.exists(self.path_of(frame))]
        # (frame packs are NOT made resident: a directory holds any number of them, 9 MB each at the reference's size.  A pack is read when its
        #  frame is taken -- inside the clock, under phase_seconds["inputs"] -- and dropped once its row is reset)
        self.inputs = {} if args.frames_dir else {frame: synthetic_frame_inputs(self.device, frame, views_of(frame, args.view_counts),
                                                                                instances_of(frame, args.instance_counts), args.height, args.width, args.label_views,
                                                                                images=bool(self.photometric)) for frame in mine}
        self.slots, self.batch = queue.Queue(), None
        self.setup_seconds, self.graphs_per_slot, self.unsuitable_founders = 0.0, 0, []
        # the frames a slot or batch may be founded on: this rank's own (static), or the head of the job's queue (dynamic: built here, once)
        candidates = mine if not self.queue.dynamic else [f for f in self.queue.order if not os.path.exists(self.path_of(f))][:max(args.frame_batch, 1) + 2]
        if candidates and not args.fresh_loops:
            t_setup = time.perf_counter()
            if args.frame_batch > 1:
                founders = [self.materialised(self.inputs_of(f)) for f in candidates[:args.frame_batch]]
                founders += [founders[-1]] * (args.frame_batch - len(founders))           # (fewer frames than rows: the shape is what matters)
                try:
                    # (a mixed list: rows of capacity max(list), each frame its own count -- the capacities, not the founders, fix the layout)
                    mixed, mixed_views = len(set(args.instance_counts)) > 1, len(set(args.view_counts)) > 1
                    self.batch = optimization.FrameBatch(founders, self.optimization_config(), self.device,
                                                         max_instances=max(args.instance_counts) if mixed else None,
                                                         max_views=max(args.view_counts) if mixed_views else None,
                                                         max_label_views=args.label_view_capacity, photometric=bool(self.photometric),
                                                         surface=self.wanted["surface"])
                    if self.logs:                # (before the captures: the buffers the log reads exist in every row)
                        self.batch.log_outputs(metrics=args.metrics, masks=args.masks)
                    self.unsuitable_founders += [int(candidates[min(f, len(candidates) - 1)]) for f in self.batch.unsuitable_founders]
                    tail = len(mine) % args.frame_batch if mine else 0                   # a static queue's last group is known now: capture it too
                    self.graphs_per_slot = self.batch.capture_all(actives=sorted({args.frame_batch, tail} - {0}, reverse=True))
                except optimization.UnsuitableFrameError:                                 # (not one of the founders suits the table sampler)
                    self.batch = None                                                     # every frame then runs in a loop of its own
                    self.unsuitable_founders += [int(f) for f in candidates[:args.frame_batch]]
            else:
                for _ in range(min(args.frames_in_flight, len(candidates))):
                    for founder in candidates:      # (a slot is founded on a frame that suits the table sampler its graphs will draw from)
                        try:
                            loop = optimization.FrameOptimizer(self.materialised(self.inputs_of(founder)), self.optimization_config(), self.device, graph=True, persistent=True,
                                                               max_label_views=args.label_view_capacity)
                        except optimization.UnsuitableFrameError:
                            self.unsuitable_founders.append(int(founder))
                            continue
                        if self.logs:
                            loop.log_outputs(metrics=args.metrics, masks=args.masks)
                        self.graphs_per_slot = loop.capture_all()
                        self.slots.put(loop)
                        break
            torch.cuda.synchronize()
            self.setup_seconds = time.perf_counter() - t_setup
        self.captures_before = optimization.exclusive_device_access().capture_seconds

    def _own_loop(self, frame):
        """A frame outside the slots / the batch (--fresh-loops, or importance weights that do not suit the table sampler): a loop of its own."""
        from . import optimization
        loop = optimization.FrameOptimizer(self.materialised(self.inputs_of(frame)), self.optimization_config(init_seed=self.init_seed(frame)), self.device, graph=True,
                                          max_label_views=self.args.label_view_capacity)
        if self.logs:
            loop.log_outputs(metrics=self.args.metrics, masks=self.args.masks)
        loss, payload, pending = self._finish_alone(frame, loop, loop.run(self.args.num_steps))
        loop.close()
        self._write_outputs(pending)
        return loss, payload

    def _note_photometric(self, frame, record):
        """--photometric: the frame's final photometric_loss, where its last step had the term (a residual step)."""
        if self.photometric and "photometric_loss" in record:
            self.photometric_losses[int(frame)] = float(record["photometric_loss"])

    def _finish_alone(self, frame, loop, record, health=None):
        """The end of a frame that ran alone, in a slot or in a loop of its own, `record` its last step's: its loss, the sampler's `health`
        where the caller reads it, its checkpoint payload and its outputs -> (loss, payload, pending file writes)."""
        from . import formats, optimization
        with optimization.exclusive_device_access():       # (host synchronisations and copies: refused now and then while another frame's thread captures)
            torch.cuda.current_stream().synchronize()
            loss = float(record["loss"])
            self._note_photometric(frame, record)
            if health is not None:
                health(frame, loop)
            payload = formats.checkpoint_payload(loop, step=self.args.num_steps - 1, metrics={}, host=True)
            rows = [(frame, self.path_of(frame))]
            return loss, payload, self._collect(loop, rows, [payload]) + self._collect_log(loop, rows)

    def _begin_outputs(self):
        """The clock's keys of --predictions / --masks / --metrics (None without any of them: outside the batch path such a job has no
        clock) and the rank's report of per-frame metrics."""
        keys = [key for flag, _, keys, *_ in _OUTPUTS if self.wanted[flag] for key in keys]
        keys += ["log", "log_write"] if self.logs else []
        self.phase_seconds, self.frame_metrics = dict.fromkeys(keys, 0.0) or None, {}

    def _collect_log(self, source, frames, active=None):
        """--scalar-interval / --ckpt-interval: the history and the snapshots of a group of finished frames, read from the device ONCE, here,
        inside the section that copies their checkpoints -> the pending writes of history.json and step_*.pt (the snapshot of the LAST step
        aside: the final checkpoint holds its models and metrics, and is what marks the frame as done).  The clock's `log`: the host time of
        the log launches between the replays (with the metrics and masks launches in front of them) and of these copies."""
        if not self.logs:
            return []
        import time
        from . import formats
        t0 = time.perf_counter()
        members = [source] if active is None else source.frames[:active]
        pending, last = [], self.args.num_steps - 1
        for (frame, path), loop in zip(frames, members):
            folder = os.path.dirname(path)
            if self.scalar_interval:
                pending.append(("log_write", formats.save_frame_history, (folder, formats.to_host(loop.history()))))
            if self.ckpt_interval:
                pending.append(("log_write", formats.save_frame_snapshots, (folder, formats.snapshot_payloads(loop.snapshots()), (last,))))
            self.phase_seconds["log"] += loop.log_seconds
            loop.log_seconds = 0.0
        self.phase_seconds["log"] += time.perf_counter() - t0
        return pending

    def _save_final(self, payload, path):
        """A frame's final checkpoint -- with --select: written under a pending name, so that it competes (select_model copies the winner
        to model.pt), and renamed last: the frame counts as done only when everything else of it is there."""
        from . import formats
        if not self.select:
            return formats.atomic_torch_save(payload, path)
        folder = os.path.dirname(path)
        pending = os.path.join(folder, "pending_" + os.path.basename(path))
        formats.atomic_torch_save(payload, pending)
        formats.select_model(folder, self.select[0], maximum=self.select[1])
        os.replace(pending, path)

    def _collect(self, source, frames, payloads, active=None):
        """What the flags ask of a group of finished frames, inside the section that copies their checkpoint `payloads`: `source` is the
        loop of ONE frame, or the batch whose first `active` rows hold the `frames` = [(frame, checkpoint path)].  In the order of `_OUTPUTS`,
        each ONE vsrd_frame_* call for the group and its copies to the host: --predictions, the labels; --group-predictions, the labels in
        every frame's own group; --masks, the target view's predicted masks, and every payload's metric mask_iou (the mean over its
        instances); --surface, the target view's dense surface render; --metrics, the reference's six metrics into the payload's `metrics`
        and the rank's report, for every frame that had 3-D ground truth.  Returns the pending file writes for `_write_outputs`."""
        import time
        pending = []
        for flag, name, _, each, how in _OUTPUTS:
            t0, arguments = time.perf_counter(), how(self, source, frames, active) if self.wanted[flag] else None
            if arguments is not None:
                entries = [getattr(source, name)(**arguments)] if active is None else getattr(source, name)(active=active, **arguments)
                for (frame, path), entry, payload in zip(frames, entries, payloads):
                    each(self, pending, frame, os.path.dirname(path), entry, payload)
                self.phase_seconds[name] += time.perf_counter() - t0
        return pending

    def _write_outputs(self, pending):
        """The label and mask files `_collect` left pending -- BEFORE the frames' checkpoints: the final checkpoint is what marks a frame as
        done (pending_frames), so a frame that has one has its files."""
        import time
        for key, save, arguments in pending:
            t0 = time.perf_counter()
            save(*arguments)
            self.phase_seconds[key] += time.perf_counter() - t0

    def run(self):
        from . import optimization
        args, losses, fallbacks, unhealthy = self.args, {}, [], []

        def health(frame, loop):
            # the device sampler's sticky flags, read at the END of a frame (a slot's next reset() rebuilds the table and clears them)
            if loop.ray_table is not None and loop.ray_table.incomplete() or loop.workspace.sampler_overflowed(self.device):
                unhealthy.append(int(frame))
                import warnings
                warnings.warn(f"frame {int(frame)}: some ray draw of this frame ran out of picks or overflowed its candidate list: those draws repeat "
                              "rays / are not reproducible (csrc/ray_sampling.h)", RuntimeWarning)

        def optimise(frame):
            slot = self.slots.get() if self._have_slots else None      # (--fresh-loops, or no frame could found a slot)
            try:
                inputs = self.inputs_of(frame)
                # (a slot serves frames of its founder's shape: a frame of another instance or view count runs in a loop of its own)
                if (slot is None or self.count_of(inputs) != slot.num_instances or self.views_of(inputs) != slot.num_views
                        or not slot.reset(inputs, init_seed=self.init_seed(frame))):
                    fallbacks.append(int(frame))
                    losses[frame], payload = self._own_loop(frame)
                    return payload
                losses[frame], payload, pending = self._finish_alone(frame, slot, slot.run(args.num_steps), health)
                self._write_outputs(pending)
                return payload
            finally:
                if slot is not None:
                    self.slots.put(slot)

        self._begin_outputs()                   # (the batch path keeps a clock of its own, with these keys added)
        self._have_slots = not args.fresh_loops and not self.slots.empty()
        if self.batch is not None:
            done = self._run_batches(losses, fallbacks, health)
        else:
            done = run_frames(self.queue, optimise, self.path_of, frames_in_flight=args.frames_in_flight, save=self._save_final)
        torch.cuda.synchronize()
        taken = len(self.queue.taken)
        return dict(frames=len(done), skipped=taken - len(done), frames_done=sorted(int(f) for f in done),
                    gate_capture_seconds=optimization.exclusive_device_access().capture_seconds - self.captures_before,
                    slot_setup_seconds=self.setup_seconds, graphs_per_slot=self.graphs_per_slot, final_losses={int(f): losses[f] for f in sorted(losses)},
                    frames_outside_slots=sorted(fallbacks), unsuitable_founders=self.unsuitable_founders, frames_with_unhealthy_draws=sorted(unhealthy),
                    phase_seconds=self.phase_seconds, final_photometric_losses=dict(sorted(self.photometric_losses.items())),
                    **({"frame_metrics": self.frame_metrics} if args.metrics else {}))

    def _run_batches(self, losses, fallbacks, health):
        """Groups of --frame-batch frames through the FrameBatch: reset row by row, ONE graph replay per (four) step(s) for the whole group,
        then the group's checkpoints.  Frames the batch cannot take (their weights do not suit its table sampler) run alone afterwards."""
        import time
        from . import formats, optimization
        args, batch, done = self.args, self.batch, []
        clock = self.phase_seconds = dict(inputs=0.0, reset=0.0, steps=0.0, checkpoint_copy=0.0, checkpoint_write=0.0, **(self.phase_seconds or {}))
        while True:
            group = pending_frames(self.queue.take(args.frame_batch), self.path_of)
            if not group:
                if self.queue.dynamic and len(self.queue.taken) < len(self.queue.order) or not self.queue.dynamic and self.queue.cursor < len(self.queue.mine):
                    continue                                        # (a group whose frames were all finished by an earlier attempt)
                break
            rows, alone = [], []
            for frame, path in group:
                t0 = time.perf_counter()
                inputs = self.inputs_of(frame)
                t1 = time.perf_counter()
                (rows if batch.reset(len(rows), inputs, init_seed=self.init_seed(frame)) else alone).append((frame, path))
                clock["inputs"] += t1 - t0
                clock["reset"] += time.perf_counter() - t1
            if rows:
                t0 = time.perf_counter()
                batch.run(args.num_steps, active=len(rows))
                with optimization.exclusive_device_access():
                    torch.cuda.current_stream().synchronize()
                    t1 = time.perf_counter()
                    payloads = []
                    for row, (frame, path) in enumerate(rows):
                        losses[frame] = float(batch.outputs(row)["loss"])
                        self._note_photometric(frame, batch.outputs(row))
                        health(frame, batch.frames[row])
                        payloads.append(formats.checkpoint_payload(batch.frames[row], step=args.num_steps - 1, metrics={}, host=True))
                    t2 = time.perf_counter()
                    pending = self._collect(batch, rows, payloads, active=len(rows)) + self._collect_log(batch, rows, active=len(rows))
                self._write_outputs(pending)
                t3 = time.perf_counter()
                for (frame, path), payload in zip(rows, payloads):
                    self._save_final(payload, path)
                    done.append(frame)
                clock["steps"] += t1 - t0
                clock["checkpoint_copy"] += t2 - t1
                clock["checkpoint_write"] += time.perf_counter() - t3
            for frame, path in alone:
                fallbacks.append(int(frame))
                losses[frame], payload = self._own_loop(frame)
                self._save_final(payload, path)
                done.append(frame)
        return done


class _SleepWork:
    """`--selftest`: a frame is a sleep and a small checkpoint.  `--selftest-fail RANK:FRAMES` makes that rank die (exit code 23, no
    clean-up, no goodbye to the process group) on attempt 0 once it has finished FRAMES frames.  `--selftest-spread X`: frame j costs
    --selftest-seconds x (1 + X u_j), u_j in [0, 1) a hash of j -- frames of unequal cost, what a static split balances badly."""

    def __init__(self, args, manifest, rank, queue):
        self.args, self.manifest, self.rank, self.queue = args, manifest, rank, queue
        self.fail_rank, self.fail_after = (int(v) for v in args.selftest_fail.split(":")) if args.selftest_fail else (-1, 0)
        self.hang_rank, self.hang_after = (int(v) for v in args.selftest_hang.split(":")) if args.selftest_hang else (-1, 0)

    def path_of(self, frame):
        return os.path.join(self.manifest["out"], f"frame_{int(frame):06d}", "step_final.pt")

    def prepare(self):
        os.makedirs(self.manifest["out"], exist_ok=True)

    def cost(self, frame):
        return self.args.selftest_seconds * (1.0 + self.args.selftest_spread * random.Random(1000 + int(frame)).random())

    def run(self):
        import time
        args, finished = self.args, []

        def optimise(frame):
            if args.attempt == 0 and self.rank == self.fail_rank and len(finished) >= self.fail_after:
                os._exit(23)
            if args.attempt == 0 and self.rank == self.hang_rank and len(finished) >= self.hang_after:
                time.sleep(1.0e6)
            time.sleep(self.cost(frame))
            finished.append(frame)
            with open(os.path.join(self.manifest["out"], "completed.log"), "a") as log:      # (O_APPEND: one short line per frame, whole)
                log.write(f"{int(frame)} {args.attempt} {self.rank}\n")
            return dict(frame=int(frame), attempt=args.attempt, rank=self.rank)

        done = run_frames(self.queue, optimise, self.path_of, frames_in_flight=1)
        return dict(frames=len(done), skipped=len(self.queue.taken) - len(done), frames_done=sorted(int(f) for f in done), gate_capture_seconds=0.0, slot_setup_seconds=0.0, graphs_per_slot=0, final_losses={},
                    frames_outside_slots=[], unsuitable_founders=[], frames_with_unhealthy_draws=[])


DEFAULT_FRAME_BATCH = 16


def effective_frame_batch(requested: int, total_frames: int, world_size: int) -> int:
    """Frames one rank steps together: what was asked for, but never more than a rank's share of the job -- groups are handed out whole
    (FrameQueue.take), so 32 frames in batches of 16 would occupy two of eight ranks.  Every rank computes the same number."""
    if requested <= 1:
        return 1
    share = -(-max(int(total_frames), 1) // max(int(world_size), 1))
    return max(1, min(int(requested), share))


def mean_frame_metrics(reports):
    """--metrics, the job's line: the mean of each metric over the frames (of every rank's report) that had ground truth, and their number."""
    from . import formats
    frames = [named for report in reports for named in (report.get("frame_metrics") or {}).values()]
    means = {name: sum(named[name] for named in frames) / len(frames) for name in formats.FRAME_METRIC_NAMES} if frames else {}
    return {"frame_metrics": means, "frame_metrics_frames": len(frames)}


def parse_select(text):
    """--select METRIC[,METRIC...][:max|:min] -> ([metrics], maximum), or None for an empty string; ValueError otherwise."""
    if not text:
        return None
    names, _, order = text.partition(":")
    metrics = [name.strip() for name in names.split(",")]
    if order not in ("", "max", "min") or not all(re.fullmatch(r"\w+", name) for name in metrics):
        raise ValueError(f"--select {text!r}: expected METRIC[,METRIC...][:max|:min]")
    return metrics, order == "max"


def parse_instances(text):
    """--instances: one count (every frame) or a comma list -- frame j has list[j % len(list)] instances (instances_of)."""
    try:
        counts = [int(x) for x in str(text).split(",")]
    except ValueError:
        raise SystemExit(f"--instances: an integer or a comma list of integers, got {text!r}")
    if not counts or any(not 1 <= n <= 64 for n in counts):
        raise SystemExit(f"--instances: counts of 1..64, got {text!r}")
    return counts


def instances_of(frame, counts):
    """The instance count of frame number `frame`: a pure function of the frame number (the same on every rank and after a restart)."""
    return int(counts[int(frame) % len(counts)])


def parse_views(text):
    """--views: one count (every frame) or a comma list -- frame j has list[j % len(list)] views (views_of)."""
    try:
        counts = [int(x) for x in str(text).split(",")]
    except ValueError:
        raise SystemExit(f"--views: an integer or a comma list of integers, got {text!r}")
    if not counts or any(not 1 <= v <= 32 for v in counts):
        raise SystemExit(f"--views: counts of 1..32, got {text!r}")
    return counts


def views_of(frame, counts):
    """The view count of frame number `frame`: list[frame % len(list)], a pure function of the frame number like instances_of -- and
    independent of the instance list's cycle (each list cycles with its own length)."""
    return int(counts[int(frame) % len(counts)])


def main(argv=None):
    """Optimise K synthetic frames, sharded over the ranks, each rank keeping `--frames-in-flight` frames on its GPU at a time with
    ``FrameOptimizer(graph=True)``; checkpoints through formats.checkpoint_payload (atomic, restartable: a frame whose final checkpoint
    exists is skipped, main.py:134-136).  Rank 0 broadcasts the manifest, the ranks start behind an ordered barrier, and rank 0 prints
    ONE JSON line: whole-job frames/s (K over the slowest rank's barrier-to-barrier time), frames/s per GPU, every rank's own time."""
    import argparse
    import json
    import sys
    import tempfile
    import time
    parser = argparse.ArgumentParser(prog="python -m vsrd_amd.launcher")
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--frames", type=int, default=0, help="frames of the whole job (default: two rounds of --frames-in-flight per process)")
    parser.add_argument("--frames-in-flight", type=int, default=1,
                        help="frames optimised at the same time by ONE process (one host thread, one stream and one persistent frame slot each; "
                             "1 = no threads at all).  Round 5, one box, split-bf16 MLP: 0.82 / 0.86 / 0.89 frames/s with 1 / 3 / 5 in one process")
    parser.add_argument("--frame-batch", type=int, default=None,
                        help="frames ONE process optimises in lock-step, every launch of a step covering all of them (optimization.FrameBatch; "
                             "include/vsrd_hip.h 'frame batches'): what fills the GPU from one RCCL rank.  1: one frame per launch chain (frame slots, "
                             "--frames-in-flight / --procs-per-gpu: the round-5 layouts).  Default: %d, or 1 when one of those layouts is asked for "
                             "(--frames-in-flight > 1, --procs-per-gpu > 1, --fresh-loops) or for a selftest" % DEFAULT_FRAME_BATCH)
    parser.add_argument("--procs-per-gpu", type=int, default=None,
                        help="rank processes per GPU (local ranks P g .. P g + P - 1 use GPU g); default 1 -- one RCCL rank per GPU -- or, under "
                             "torchrun, LOCAL_WORLD_SIZE / visible GPUs.  Round 5's layout was P = 2 with --frame-batch 1: the kernels of two processes "
                             "overlap better than the streams of one (1.02-1.11 frames/s against 0.82, profiles/r05/frames_per_s.txt); RCCL refuses two "
                             "ranks on one device, so with P > 1 the control plane -- barriers, manifest broadcast, gather of the report; nothing else "
                             "crosses ranks -- is gloo")
    parser.add_argument("--queue", choices=("static", "dynamic", "auto"), default="auto",
                        help="static: frame j of the seeded permutation to rank j mod world, inputs resident before the clock.  dynamic: the ranks take "
                             "their next group of frames from ONE queue (an atomic counter on rank 0's TCPStore): frames of unequal cost leave no rank idle "
                             "for more than one group; inputs are built when a frame is taken.  auto: dynamic when the job has more than one rank")
    parser.add_argument("--adjoint-item-slots", type=int, default=0,
                        help="OptimizationConfig.mlp_adjoint_item_slots (vsrd_render_config::adjoint_slots_per_item): 0 = planned (4 for one frame of 1000 rays; "
                             "a batch picks FrameBatch.item_slots).  A frame's trajectory is bit-identical alone and in a batch for equal numbers")
    parser.add_argument("--fp32-mlp", action="store_true", help="the residual MLP's products on the exact-fp32 matrix instruction instead of split bf16")
    parser.add_argument("--photometric", type=float, default=0.0, metavar="W",
                        help="loss_weights['photometric_loss'] = W (default 0: the term is off): the multi-view patch-correlation term in every residual "
                             "step, in frame batches too (optimization.FrameBatch(..., photometric=True)).  Synthetic frames then carry images "
                             "(synthetic.synthetic_images); --frames-dir packs must carry the member `images` (tools/make_frame_packs.py --images)")
    parser.add_argument("--frames-dir", default="",
                        help="optimise the frame packs of this directory (vsrd_amd/frames.py; tools/make_frame_packs.py writes synthetic ones) instead of "
                             "synthetic frames: frame j is the j-th of its sorted *.npz files, --frames defaults to all of them, views / image size / "
                             "instance counts are the packs' own and may differ from pack to pack, the image size may not (not to be combined with --views, --instances, "
                             "--height, --width)")
    parser.add_argument("--views", type=str, default=None,
                        help="views per frame: one count, or a comma list (frame j gets list[j %% len(list)], whatever the --instances list gives it: "
                             "each list cycles with its own length); with --frame-batch > 1 a mixed list runs in batches of view capacity max(list) "
                             "(optimization.FrameBatch(max_views=...)); 1..32, default 17")
    parser.add_argument("--instances", type=str, default=None,
                        help="instances per frame: one count, or a comma list (frame j gets list[j %% len(list)]); with --frame-batch > 1 a mixed "
                             "list runs in batches of capacity max(list) (optimization.FrameBatch(max_instances=...)); default 8")
    parser.add_argument("--rays", type=int, default=1000)
    parser.add_argument("--samples", type=int, default=100)
    parser.add_argument("--num-steps", type=int, default=3000)
    parser.add_argument("--warmup-steps", type=int, default=1000)
    parser.add_argument("--height", type=int, default=None, help="default 376")
    parser.add_argument("--width", type=int, default=None, help="default 1408")
    parser.add_argument("--out", default="", help="checkpoint directory (default: a temporary one)")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--predictions", action="store_true",
                        help="after a frame's steps, write its pseudo-labels next to its checkpoint: predictions/view_VV.json for every view "
                             "(tools/kitti_360/make_predictions.py) and labels/view_00.txt, the target view's KITTI label lines "
                             "(convert_predictions.py) -- vsrd_frame_labels, one launch per group of frames; with --frames-dir an end-to-end "
                             "auto-labelling run.  Not with --selftest")
    parser.add_argument("--group-predictions", action="store_true",
                        help="after a frame's steps, write its pseudo-labels in the frames of its GROUP (the frames whose instance set equals the "
                             "target's: what tools/kitti_360/make_predictions.py labels and a detector is trained on) before its checkpoint: "
                             "group/predictions/<id>.json and group/labels/<id>.txt for every group frame -- vsrd_frame_group_labels, one call per "
                             "group of frames.  Needs --out and frames that carry a group: --frames-dir packs with the label_* members, or "
                             "synthetic frames with --label-views; not with --selftest")
    parser.add_argument("--label-views", type=int, default=0,
                        help="synthetic frames carry a group of this many label views (synthetic.synthetic_group); packs carry their own")
    parser.add_argument("--masks", action="store_true",
                        help="after a frame's steps, render the target view's dense predicted instance masks (scripts/main.py:1011-1061: volume_masks "
                             "x surface_masks) -- vsrd_frame_masks, one launch per group of frames -- write them bit-packed to masks/view_00.npz next "
                             "to the frame's checkpoint and store their mean IoU against the masks the frame was fitted to as the checkpoint's "
                             "metric `mask_iou`; with --ckpt-interval every step_*.pt carries it too, and --select mask_iou:max picks among "
                             "them.  Needs --out; not with --selftest")
    parser.add_argument("--surface", action="store_true",
                        help="after a frame's steps, render the target view's dense surface -- range, owning instance, shadow and a shaded colour image "
                             "of the fitted field, laid over the frame's photograph when the frame carries its images (scripts/main.py:1028-1041) -- "
                             "vsrd_frame_surface, one launch per group of frames -- and write surface/view_00.npz and surface/view_00.png next to the "
                             "frame's checkpoint.  Needs --out; not with --selftest")
    parser.add_argument("--surface-light", default="",
                        help="X,Y,Z: the direction the light of --surface travels, in the rectified camera frame (x right, y down, z forward).  "
                             "Default 0.3,1,0.6: from above and behind the camera, a little from the left")
    parser.add_argument("--metrics", action="store_true",
                        help="after a frame's steps, evaluate its boxes against the frame's 3-D ground truth (FrameInputs.boxes_3d / a frame pack's "
                             "boxes_3d; synthetic frames carry their true boxes) -- vsrd_frame_metrics, one launch per group of frames -- and store the "
                             "reference's iou_3d, iou_bev, accuracy_3d_25, accuracy_bev_25, accuracy_3d_50, accuracy_bev_50 (scripts/main.py:870-924) in "
                             "the checkpoint's `metrics` (with --ckpt-interval in every step_*.pt too, for --select); the job's line gets their means over the frames that had ground "
                             "truth (`frame_metrics`, `frame_metrics_frames`); frames without it are skipped.  Not with --selftest")
    parser.add_argument("--scalar-interval", type=int, default=0,
                        help="every K steps log a frame's scalars on the device (the reference's scalar_intervals, 50: losses, learning rates, "
                             "annealed hyperparameters, with --metrics the six metrics) -- vsrd_frame_log between the graph replays, read once per "
                             "frame -- and write them to history.json next to the frame's checkpoint.  0: off.  Needs --out; not with --selftest")
    parser.add_argument("--ckpt-interval", type=int, default=0,
                        help="every K steps keep a snapshot of a frame's models on the device (the reference's ckpt_intervals, 500) and write them "
                             "as step_{step}.pt (step, models, metrics: with --metrics the six metrics, with --masks mask_iou) before the frame's "
                             "final checkpoint.  0: off.  Needs --out; not with --selftest")
    parser.add_argument("--select", default="",
                        help="METRIC[,METRIC...][:max|:min] (default :min): copy the frame's step_*.pt with the best mean of these metrics to "
                             "model.pt (the rule of tools/select_model.py; a tie keeps the earliest step), which make_predictions.py "
                             "--ckpt_filename model.pt picks up.  Needs --out; not with --selftest")
    parser.add_argument("--ranks-share-gpu", action="store_true",
                        help="TEST ONLY: every rank on cuda:0, gloo rendezvous (RCCL refuses two ranks on one device); the line says so")
    parser.add_argument("--fresh-loops", action="store_true",
                        help="A/B: build a new FrameOptimizer (construction, eager warm-up steps, ~10 captures) for every frame, as round 4 did, "
                             "instead of the persistent frame slots whose graphs are captured once at start-up")
    parser.add_argument("--max-restarts", type=int, default=2,
                        help="without torchrun around it, the launcher supervises its ranks: when one dies, all are started again as fresh "
                             "processes, this many times at most; finished frames are skipped (0 with --gpus 1: no supervisor process)")
    parser.add_argument("--stall-timeout", type=float, default=0.0,
                        help="supervisor: seconds without anything new in the checkpoint directory after which the ranks are taken for hung, ended and "
                             "restarted like after a dead rank; 0 = never (the default).  The clock starts with the attempt and starts over when rank 0 "
                             "has finished its set-up (it touches the directory) and with every checkpoint, so the value must exceed both the start-up (library "
                             "build, inputs, graph capture: tens of seconds) and the time of one group of --frame-batch frames")
    parser.add_argument("--attempt", type=int, default=0, help=argparse.SUPPRESS)          # set by the supervisor: restarts so far
    parser.add_argument("--selftest", action="store_true",
                        help="no rendering, no GPU: a frame is a sleep of --selftest-seconds and a small checkpoint (gloo, CPU) -- the supervisor, "
                             "the sharding, the rank -> device map, the skip-if-done guard and the report, for tests/test_launcher.py; the line says so")
    parser.add_argument("--selftest-seconds", type=float, default=0.05)
    parser.add_argument("--selftest-spread", type=float, default=0.0, help="frame j costs --selftest-seconds x (1 + spread x u_j), u_j in [0, 1) fixed per frame")
    parser.add_argument("--selftest-fail", default="", help="RANK:FRAMES -- on attempt 0 that rank dies (exit code 23) once it has finished FRAMES frames")
    parser.add_argument("--selftest-hang", default="", help="RANK:FRAMES -- on attempt 0 that rank hangs (sleeps for ever) once it has finished FRAMES frames")
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parser.parse_args(argv)
    if args.predictions and args.selftest:
        raise SystemExit("--predictions writes the labels of optimised frames; --selftest optimises none: drop one of --selftest, --predictions")
    if args.masks and args.selftest:
        raise SystemExit("--masks renders the masks of optimised frames; --selftest optimises none: drop one of --selftest, --masks")
    if args.surface and args.selftest:
        raise SystemExit("--surface renders the surface of optimised frames; --selftest optimises none: drop one of --selftest, --surface")
    if args.surface and not args.out:
        raise SystemExit("--surface writes surface/view_00.npz and surface/view_00.png next to every frame's checkpoint: it needs --out")
    try:
        args.surface_light = parse_light(args.surface_light)
    except ValueError as error:
        raise SystemExit(str(error))
    if args.surface_light is not None and not args.surface:
        raise SystemExit("--surface-light sets the light of --surface: add --surface or drop it")
    if args.metrics and args.selftest:
        raise SystemExit("--metrics evaluates the boxes of optimised frames; --selftest optimises none: drop one of --selftest, --metrics")
    for flag, value in (("--scalar-interval", args.scalar_interval), ("--ckpt-interval", args.ckpt_interval), ("--select", args.select)):
        if value and args.selftest:
            raise SystemExit(f"{flag} logs optimised frames; --selftest optimises none: drop one of --selftest, {flag}")
        if value and not args.out:
            raise SystemExit(f"{flag} writes history.json, step_*.pt and model.pt next to every frame's checkpoint: it needs --out")
    if args.photometric and args.selftest:
        raise SystemExit("--photometric is a term of optimised frames' loss; --selftest optimises none: drop one of --selftest, --photometric")
    if not (args.photometric >= 0.0 and args.photometric < float("inf")):
        raise SystemExit(f"--photometric: a finite weight >= 0 (0: off), got {args.photometric}")
    if args.scalar_interval < 0 or args.ckpt_interval < 0:
        raise SystemExit("--scalar-interval and --ckpt-interval must be at least 0 (0: off)")
    try:
        parse_select(args.select)
    except ValueError as error:
        raise SystemExit(str(error))
    if args.group_predictions and args.selftest:
        raise SystemExit("--group-predictions writes the labels of optimised frames; --selftest optimises none: drop one of --selftest, --group-predictions")
    if args.group_predictions and not args.out:
        raise SystemExit("--group-predictions writes group/predictions/<id>.json and group/labels/<id>.txt next to every frame's checkpoint: it needs --out")
    if not 0 <= args.label_views <= 4096:
        raise SystemExit("--label-views must be 0..4096")
    if args.label_views and args.frames_dir:
        raise SystemExit("--frames-dir: the packs carry their own groups; drop --label-views")
    if args.group_predictions and not args.frames_dir and not args.label_views:
        raise SystemExit("--group-predictions needs frames that carry a group: --frames-dir packs with the label_* members, or synthetic frames with --label-views L")
    if args.masks and not args.out:
        raise SystemExit("--masks writes masks/view_00.npz and a mask_iou metric next to every frame's checkpoint: it needs --out")
    if args.frames_dir:
        given = [flag for flag, value in (("--views", args.views), ("--instances", args.instances), ("--height", args.height), ("--width", args.width)) if value is not None]
        if given:
            raise SystemExit(f"--frames-dir: the packs carry their own views, image size and instance counts; drop {', '.join(given)}")
        # (the supervisor starts its ranks in the repository root: they get the directory as an absolute path, in a flag of its own
        #  behind the caller's -- the last one counts)
        args.frames_dir = os.path.abspath(args.frames_dir)
        argv = argv + ["--frames-dir", args.frames_dir]
        if "RANK" not in os.environ:          # (a job nobody could run ends here, before any rank starts; rank 0 reads the counts again for the manifest)
            files, _ = scan_frames_dir(args.frames_dir, args.frames)
            if args.group_predictions:
                scan_label_views(files)
            if args.photometric:
                scan_images(files)
    args.height, args.width = (default if value is None else value for value, default in ((args.height, 376), (args.width, 1408)))
    args.view_counts = parse_views("17" if args.views is None else args.views)
    args.views = args.view_counts[0] if len(args.view_counts) == 1 else ",".join(str(v) for v in args.view_counts)
    args.instances = "8" if args.instances is None else args.instances
    args.instance_counts = parse_instances(args.instances)
    args.instances = args.instance_counts[0] if len(args.instance_counts) == 1 else args.instances
    if not 1 <= args.frames_in_flight <= (4 if args.fresh_loops else 8):
        # (round 4, a new loop per frame: five and more frames on one device ended in a memory fault or a segmentation fault inside torch / HIP
        #  within seconds -- construction and eager warm-up steps of that many threads next to a capture.  Frame slots capture nothing once
        #  the workers run; eight is what was tried.)
        raise SystemExit("--frames-in-flight must be 1..8 (1..4 with --fresh-loops)")
    under_launcher = "RANK" in os.environ and "--attempt" not in argv          # (torchrun around us: the supervisor's own ranks carry --attempt)
    if args.procs_per_gpu is None:
        # (a `torchrun --nproc-per-node <GPUs>` command must mean one rank per GPU, whatever this launcher's own default is)
        args.procs_per_gpu = 1
        if under_launcher and not args.selftest and not args.ranks_share_gpu:
            local_world, devices = int(os.environ.get("LOCAL_WORLD_SIZE", "1")), max(torch.cuda.device_count(), 1)
            args.procs_per_gpu = max(local_world // devices, 1)
    if under_launcher and not args.selftest and not args.ranks_share_gpu:
        local_world, devices = int(os.environ.get("LOCAL_WORLD_SIZE", "1")), max(torch.cuda.device_count(), 1)
        if local_world % args.procs_per_gpu or local_world // args.procs_per_gpu > devices:
            raise SystemExit(f"{local_world} local ranks do not map onto {devices} visible GPU(s) with --procs-per-gpu {args.procs_per_gpu}: "
                             "--nproc-per-node must be GPUs x procs-per-gpu")
    if under_launcher and not args.out and int(os.environ.get("TORCHELASTIC_MAX_RESTARTS", "0") or 0) > 0:
        # (a restarted attempt must find the checkpoints of the one before: rank 0's temporary directory would be a new one every time)
        raise SystemExit("torchrun --max-restarts needs --out: the skip-if-done guard works on a checkpoint directory that outlives an attempt")
    if not (1 <= args.procs_per_gpu <= 4 and (args.selftest or args.procs_per_gpu * args.frames_in_flight <= 6 or args.procs_per_gpu == 1)):
        # (four processes with two frames each took 190 s for 32 frames where 4 x 1 and 2 x 3 take 16 and 26: profiles/r05/frames_per_s.txt)
        raise SystemExit("--procs-per-gpu must be 1..4 with at most 6 frames in flight per GPU between them")
    if args.frame_batch is None:
        args.frame_batch = 1 if (args.frames_in_flight > 1 or args.procs_per_gpu > 1 or args.fresh_loops or args.selftest) else DEFAULT_FRAME_BATCH
    if not 1 <= args.frame_batch <= 64:
        raise SystemExit("--frame-batch must be 1..64")
    if args.frame_batch > 1 and (args.frames_in_flight > 1 or args.fresh_loops):
        raise SystemExit("--frame-batch B > 1 is ONE thread stepping B frames together: use it with --frames-in-flight 1 and without --fresh-loops")
    if args.ranks_share_gpu:
        args.procs_per_gpu = 1               # (the test flag puts every rank on cuda:0 by itself)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # __graft_entry__.build lives at the repo root
    if root not in sys.path:
        sys.path.insert(0, root)
    if "RANK" not in os.environ and (args.gpus * args.procs_per_gpu > 1 or args.max_restarts > 0):
        return _supervise(argv, args)
    return _rank_main(args)


def _rank_main(args):
    import json
    import sys
    import tempfile
    import time
    use_gpu = not args.selftest
    procs = args.procs_per_gpu
    # RCCL only when every rank has a device of its own
    share = args.ranks_share_gpu or procs > 1
    if args.ranks_share_gpu:
        os.environ["LOCAL_RANK"] = "0"
    local_device = int(os.environ.get("LOCAL_RANK", "0")) // procs
    if use_gpu:
        if not torch.cuda.is_available():
            raise SystemExit("vsrd_amd.launcher optimises frames on HIP devices: no GPU visible, and vsrd_amd has no CPU fallback")
        rank, world, device = init_process_group(backend="gloo" if share else None, ranks_per_device=procs)
        import __graft_entry__
        if rank == 0:
            __graft_entry__.build()
        barrier()
    else:
        rank, world, device = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), None
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29500")
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    packs = shapes = label_views = None
    if args.frames_dir and rank == 0:        # rank 0 alone lists the directory and opens the files for their counts: the job is what ITS list says
        packs, shapes = scan_frames_dir(args.frames_dir, args.frames)
        args.frames = len(packs)
        if args.group_predictions:
            label_views = scan_label_views(packs)
    total = args.frames or (2 * max(args.frames_in_flight, args.frame_batch) * world if use_gpu else 4 * world)
    out_dir = args.out or (tempfile.mkdtemp(prefix="vsrd_frames_") if rank == 0 else None)
    dynamic = args.queue == "dynamic" or (args.queue == "auto" and world > 1)
    store = None
    store_port = 0
    if dynamic:                              # rank 0 serves the queue's counter; the port travels in the manifest
        host = os.environ.get("MASTER_ADDR", "127.0.0.1")
        if rank == 0:
            store = dist.TCPStore(host, 0, world, is_master=True, wait_for_workers=False)
            store_port = store.port
    manifest = broadcast_manifest(dict(frames=list(range(total)), seed=args.seed, out=out_dir, store_port=store_port, attempt=args.attempt,
                                       packs=packs, pack_shapes=shapes, pack_label_views=label_views) if rank == 0 else None)      # (pack_shapes: every pack's (V, H, W, N))
    total = len(manifest["frames"])          # (every rank sizes the job from the manifest)
    args.frame_batch = effective_frame_batch(args.frame_batch, total, world)
    if manifest.get("packs"):                # frame j's count is its pack's: instances_of(j, counts) with one entry per frame
        args.height, args.width = manifest["pack_shapes"][0][1:3]
        args.instance_counts = [int(shape[3]) for shape in manifest["pack_shapes"]]
        args.instances = ",".join(str(n) for n in sorted(set(args.instance_counts)))
        args.view_counts = [int(shape[0]) for shape in manifest["pack_shapes"]]
        args.views = ",".join(str(v) for v in sorted(set(args.view_counts)))
    # the label-view capacity of every loop and row: the job's largest L with --group-predictions, else no loop keeps a group
    args.label_view_capacity = (max(manifest["pack_label_views"]) if manifest.get("pack_label_views") else args.label_views) if args.group_predictions else 0
    if not manifest["out"]:
        raise SystemExit("no checkpoint directory (--out; the supervisor supplies one)")
    if dynamic and rank != 0:
        store = dist.TCPStore(os.environ.get("MASTER_ADDR", "127.0.0.1"), int(manifest["store_port"]), world, is_master=False)
    queue = FrameQueue(manifest["frames"], rank, world, seed=manifest["seed"], store=store, key=f"vsrd_next_frame_{manifest['attempt']}")
    ordered(lambda r: print(f"[rank {r}/{world}] " + (f"selftest, device {local_device}" if args.selftest else str(device)) +
                            (": frames from the job's queue" if dynamic else f": frames {queue.mine}"), file=sys.stderr, flush=True))
    work = _SleepWork(args, manifest, rank, queue) if args.selftest else _RenderWork(args, manifest, device, queue)
    work.prepare()
    if rank == 0:                            # the supervisor's stall clock starts over at the first fence: the directory's own time stamp
        os.makedirs(manifest["out"], exist_ok=True)
        os.utime(manifest["out"], None)

    def fence():
        barrier()
        if use_gpu:
            torch.cuda.synchronize()

    fence()
    t0 = time.perf_counter()
    report = work.run()
    own = time.perf_counter() - t0
    fence()
    elapsed = time.perf_counter() - t0
    losses = report["final_losses"]
    report.update(rank=rank, device=local_device, own_seconds=own, elapsed_seconds=elapsed, mean_final_loss=(sum(losses.values()) / len(losses)) if losses else None)
    gathered = [report]
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, report)
    if rank == 0:
        slowest = max(r["elapsed_seconds"] for r in gathered)
        frames_done = sum(r["frames"] for r in gathered)
        n_gpus = len(gathered) if args.ranks_share_gpu else max(len(gathered) // procs, 1)       # (--ranks-share-gpu: the test's line counts ranks, as before)
        if args.selftest:
            line = {"metric": "launcher selftest: no rendering, NOT a measurement", "value": 0.0, "unit": "none", "n_gpus": n_gpus, "ranks": len(gathered),
                    "procs_per_gpu": procs, "rank_devices": [r["device"] for r in gathered], "frames": frames_done,
                    "frames_skipped_as_done": sum(r["skipped"] for r in gathered), "per_rank_frames": [r["frames"] for r in gathered],
                    "restarts": args.attempt, "max_restarts": args.max_restarts, "queue": "dynamic" if dynamic else "static",
                    "frames_dir": args.frames_dir or None,
                    "frames_per_instances": {str(n): sum(1 for r in gathered for f in r["frames_done"] if instances_of(f, args.instance_counts) == n)
                                             for n in sorted(set(args.instance_counts))},
                    "frames_per_views": {str(v): sum(1 for r in gathered for f in r["frames_done"] if views_of(f, args.view_counts) == v)
                                         for v in sorted(set(args.view_counts))},
                    "per_rank_seconds": [r["own_seconds"] for r in gathered],
                    "rank_finish_spread_seconds": max(r["own_seconds"] for r in gathered) - min(r["own_seconds"] for r in gathered),
                    "config": {"workload": f"sleep({args.selftest_seconds} s x (1 + {args.selftest_spread} u)) per frame on gloo / CPU", "checkpoints": manifest["out"]}}
        else:
            line = {
                "metric": "optimised target frames/s, whole job (reference: about 15 minutes per frame on a V100, README.md:128)",
                "value": frames_done / slowest, "unit": "frames/s", "n_gpus": n_gpus, "higher_is_better": True, "scaling": "weak",
                "frames": frames_done, "frames_skipped_as_done": sum(r["skipped"] for r in gathered), "seconds": slowest,
                "restarts": args.attempt, "max_restarts": args.max_restarts,     # (restarts > 0: `seconds` and `frames` are the last attempt's)
                "frames_per_s_per_gpu": frames_done / slowest / n_gpus,
                "ranks": len(gathered), "procs_per_gpu": procs, "frames_in_flight_per_process": args.frames_in_flight, "rank_devices": [r["device"] for r in gathered],
                "frame_batch": args.frame_batch,        # frames one process steps together, one launch of every kernel for all of them (optimization.FrameBatch)
                # instances per frame (frame j: instance_list[j % len]); frames done per count; the rows' capacity of a mixed batch (None: one shape)
                "instance_list": sorted(set(args.instance_counts)) if args.frames_dir else list(args.instance_counts),
                "frames_dir": args.frames_dir or None,
                "frames_per_instances": {str(n): sum(1 for r in gathered for f in r["final_losses"] if instances_of(f, args.instance_counts) == n)
                                         for n in sorted(set(args.instance_counts))},
                "batch_capacity": max(args.instance_counts) if args.frame_batch > 1 and len(set(args.instance_counts)) > 1 else None,
                # views per frame (frame j: view_list[j % len]); frames done per count; the rows' view capacity of a batch of mixed views
                "view_list": sorted(set(args.view_counts)) if args.frames_dir else list(args.view_counts),
                "frames_per_views": {str(v): sum(1 for r in gathered for f in r["final_losses"] if views_of(f, args.view_counts) == v)
                                     for v in sorted(set(args.view_counts))},
                "batch_view_capacity": max(args.view_counts) if args.frame_batch > 1 and len(set(args.view_counts)) > 1 else None,
                "control_plane": "gloo" if share else "RCCL",
                "queue": "dynamic (TCPStore counter on rank 0; inputs built when a frame is taken, inside the clock)" if dynamic else
                         "static (frame j of the seeded permutation to rank j mod world; " +
                         ("packs read when a frame is taken, inside the clock)" if args.frames_dir else "inputs resident before the clock)"),
                # the spread of the ranks' own finishing times: what a static split of unequal frames costs the job, what the queue bounds by one group
                "rank_finish_spread_seconds": max(r["own_seconds"] for r in gathered) - min(r["own_seconds"] for r in gathered),
                "mlp_products": "exact fp32 (v_mfma_f32_16x16x4_f32)" if args.fp32_mlp else "split bf16 (v_mfma_f32_16x16x32_bf16 on hi/lo parts, fp32 accumulation)",
                "per_rank_seconds": [r["own_seconds"] for r in gathered], "per_rank_frames": [r["frames"] for r in gathered],
                "seconds_per_frame_per_rank": [r["own_seconds"] / r["frames"] if r["frames"] else None for r in gathered],
                # --photometric: the term's weight (0: off) and the mean of the frames' final photometric_loss (None: no frame ended in a residual step)
                "photometric_weight": args.photometric,
                "mean_final_photometric_loss": (lambda values: sum(values) / len(values) if values else None)(
                    [v for r in gathered for v in r.get("final_photometric_losses", {}).values()]),
                "mean_final_loss": [r["mean_final_loss"] for r in gathered], "data": "frame packs" if args.frames_dir else "synthetic", "dtype": "f32",
                "final_loss_per_frame": {str(f): v for r in gathered for f, v in r["final_losses"].items()},
                # host time per frame spent capturing hipGraphs (optimization._CaptureGate): what the other frames in flight wait for
                "capture_seconds_per_frame": [r["gate_capture_seconds"] / r["frames"] if r["frames"] else None for r in gathered],
                # persistent frame slots: built and captured once per process BEFORE the clock (a job of thousands of frames pays it once)
                "frame_slots": not args.fresh_loops, "slot_setup_seconds": [r["slot_setup_seconds"] for r in gathered],
                "graphs_per_slot": [r["graphs_per_slot"] for r in gathered],
                # frames a slot could not take (their importance weights do not suit the sampling table its graphs draw from: a loop of their own, race sampler)
                # where a batched rank's time went, in seconds over its frames: building inputs (dynamic queue only), resetting rows, the steps, checkpoints
                "phase_seconds": [r.get("phase_seconds") for r in gathered],
                **({"predictions": True} if args.predictions else {}),
                **({"group_predictions": True} if args.group_predictions else {}),
                **({"masks": True} if args.masks else {}),
                **({"surface": True} if args.surface else {}),      # (--predictions: label files next to every checkpoint)
                **({"frame_log": {"scalar_interval": args.scalar_interval, "ckpt_interval": args.ckpt_interval, "select": args.select}}
                   if args.scalar_interval or args.ckpt_interval or args.select else {}),
                **(mean_frame_metrics(gathered) if args.metrics else {}),
                "frames_outside_slots": sorted(f for r in gathered for f in r["frames_outside_slots"]),
                "unsuitable_founders": sorted(f for r in gathered for f in r["unsuitable_founders"]),
                # frames in which some ray draw ran out of picks / overflowed (read at the end of each frame; RuntimeWarning on stderr)
                "frames_with_unhealthy_draws": sorted(f for r in gathered for f in r["frames_with_unhealthy_draws"]),
                "config": {"workload": f"{args.num_steps} optimisation steps per frame ({args.warmup_steps} box-only + {args.num_steps - args.warmup_steps} with the "
                                       f"residual MLP), {args.rays} rays x {args.samples} samples per step, {args.views} views of {args.height}x{args.width}, "
                                       f"{args.instances} instances, " +
                                       (f"FrameBatch: {args.frame_batch} frames per launch chain, {procs} rank process(es) per GPU (graphs captured once at start-up)"
                                        if args.frame_batch > 1 else
                                        f"FrameOptimizer(graph=True), {procs} rank process(es) per GPU x {args.frames_in_flight} frame(s) in flight each"
                                        + (" (a new loop per frame)" if args.fresh_loops else " (persistent frame slots: graphs captured once at start-up)")),
                           "parallelism": f"frames sharded over {len(gathered)} rank(s) on {n_gpus} GPU(s), no data-path collective; "
                                          + ("gloo (RCCL refuses two ranks on one device)" if share else "RCCL") + ": barriers, manifest broadcast, gather of the report",
                           "checkpoints": manifest["out"]},
            }
            if len(set(args.view_counts)) > 1:
                line["metric"] += f"; frames of {args.views} views"
            if args.ranks_share_gpu:
                line["metric"] = "ranks share ONE GPU (--ranks-share-gpu): a test of the multi-rank path, NOT a scaling measurement; " + line["metric"]
        print(json.dumps(line), flush=True)
    barrier()
    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
