"""Host batch -> device in ONE asynchronous copy: the bytes go through a pinned staging buffer (a small ring, so the host can run
ahead of the device) and land in one device buffer; callers take typed views of it or address the arrays in it.  Several small
pageable copies per step each wait for the stream to drain — on this path that alone serialised host and device."""
import numpy as np
import torch

from .engine_dense import aligned_offsets


class StagedUpload:
    def __init__(self, device, slots=4):
        self.device, self.n = torch.device(device), slots
        self.host, self.ev, self.i = [None] * slots, [None] * slots, 0
        self.kept = [None] * slots           # upload_kept: what stays on the device with each pinned slot

    def _slot(self, total):
        """the next pinned slot, grown to `total` bytes and free to be written: (its index, its bytes as a numpy view)"""
        k = self.i % self.n
        self.i += 1
        if self.host[k] is None or self.host[k].numel() < total:
            self.host[k] = torch.empty(int(total * 1.5) + 4096, dtype=torch.uint8, pin_memory=True)
            self.ev[k] = torch.cuda.Event()
            self.kept[k] = None              # (the device side is replaced together with the pinned one, and what was cached with it)
        else:
            self.ev[k].synchronize()         # the copy that last read this pinned slot has finished
        return k, self.host[k].numpy()

    def _send(self, k, dev, total):
        dev.copy_(self.host[k][:total], non_blocking=True)
        self.ev[k].record(torch.cuda.current_stream(self.device))
        return dev

    def pack(self, arrays):
        """arrays: contiguous numpy arrays.  Returns (device uint8 tensor owning the bytes, the byte offset of every array in it)."""
        offs, total = aligned_offsets([a.nbytes for a in arrays])
        total = max(total, 16)
        k, hv = self._slot(total)
        for a, o in zip(arrays, offs):
            hv[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        return self._send(k, torch.empty(total, dtype=torch.uint8, device=self.device), total), offs

    def __call__(self, arrays):
        """pack(arrays) with typed device views of the arrays in place of their offsets"""
        dev, offs = self.pack(arrays)
        views = [dev[o:o + a.nbytes].view(_TORCH[a.dtype.type]).reshape(a.shape) if a.nbytes else
                 torch.empty(a.shape, dtype=_TORCH[a.dtype.type], device=self.device) for a, o in zip(arrays, offs)]
        return dev, views

    def upload(self, buf):
        """buf: one prepared numpy uint8 buffer.  Returns a fresh device tensor with its bytes (owned by the caller)."""
        total = buf.nbytes
        k, hv = self._slot(total)
        hv[:total] = buf
        return self._send(k, torch.empty(total, dtype=torch.uint8, device=self.device), total)

    def upload_kept(self, buf):
        """The same into a device buffer that the ring slot KEEPS: steps run in order on one stream, so a copy into it is queued
        behind the step that last read it — and a slot's addresses stay the same from visit to visit.  Returns the slot's dict
        {'k': its index, 'dev': the device buffer}; the caller may keep what depends on those addresses in it (the dict is
        dropped when the slot has to grow)."""
        total = buf.nbytes
        k, hv = self._slot(total)
        hv[:total] = buf
        kept = self.kept[k]
        if kept is None:
            kept = self.kept[k] = {'k': k, 'dev': torch.empty(self.host[k].numel(), dtype=torch.uint8, device=self.device)}
        self._send(k, kept['dev'][:total], total)
        return kept


_TORCH = {np.int32: torch.int32, np.int64: torch.int64, np.float32: torch.float32, np.float64: torch.float64, np.uint8: torch.uint8}
