"""The row arena of the tests that meet the frame entry points of the C ABI by hand (test_hip_frame_labels.py, test_hip_frame_group_labels.py,
test_hip_frame_metrics.py): host memory laid out like a frame batch's rows, without vsrd_amd.optimization's allocator -- these tests exist to
meet the ABI without the product's own."""
import math

import torch


class RowArena:
    """B rows of the buffers `fields` = [(name, shape, dtype)]: every buffer at the same 256-byte aligned offset of its frame's row, rows
    `stride` bytes apart, `gap` bytes behind each row that no buffer covers.  Every int32 of `host` starts as `fill_bits`, so that what a call
    did not write is found by comparing bytes."""

    def __init__(self, fields, B, fill_bits, gap):
        self.B, self.gap, self.layout, cursor = B, gap, {}, 0
        for name, shape, dtype in fields:
            nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
            self.layout[name] = (cursor, nbytes, shape, dtype)
            cursor = (cursor + nbytes + 255) // 256 * 256
        self.stride = cursor + gap
        assert self.stride % 256 == 0
        self.host = torch.empty(B * self.stride, dtype=torch.uint8)
        self.host.view(torch.int32).fill_(fill_bits)

    def view(self, name, f=0, host=None):
        """Frame f's buffer `name` as a tensor over `host` (default: the arena's own bytes)."""
        offset, nbytes, shape, dtype = self.layout[name]
        start = f * self.stride + offset
        return (self.host if host is None else host)[start:start + nbytes].view(dtype).view(shape)

    def pointers(self, device, null=()):
        """name -> the address of frame 0's buffer in `device`, a device copy of `host` (None for the names in `null`)."""
        base = device.data_ptr()
        return lambda name: None if name in null else base + self.layout[name][0]

    def write_header(self, f, n, name="header"):
        """The two ABI-9 fields of frame f's vsrd_frame_header: n instances, a loss scale of 1."""
        header = self.view(name, f)
        header[0] = n
        header.view(torch.float32)[1] = 1.0
