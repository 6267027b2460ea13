"""Training batches cut on the device out of cases that stay in HBM (device half; opt-in).

``DataLoader3D`` (dataset_loading.py) crops every sample on the host, pads it into a page-locked batch of the loader's enlarged patch
(205^3 for a 128^3 training patch: 345 MB for four modalities and batch 2, most of it padding) and uploads that.  Here the
preprocessed cases themselves live on the device and ``e2e_loader_crop`` (csrc/loader.hip) cuts and pads the whole batch in one
launch; the host keeps the ``numpy.random`` draws, a few dozen scalars per batch.

  * ``DeviceCaseCache``: the cases, ``[C + 1, X, Y, Z]`` fp32 exactly as ``_load_case`` returns them, keyed by file path.  A case is
    uploaded the first time it is drawn and kept while the byte budget is not exceeded.  No eviction, no heuristic.
  * ``ResidentDataLoader3D``: ``DataLoader3D``'s constructor plus ``cache``; the draws are ``DataLoader3D.draw_batch``, so under one
    seed both loaders name the same patches and leave the random stream at the same position.  A case that is not resident goes
    through the same kernel: the host copies only the part of it the patch covers into a page-locked staging buffer, uploads that and
    hands the kernel the box with the offset moved by the box's corner.  The bytes of a batch therefore never depend on the budget.

There is no CPU path: without a GPU the loader refuses to be built.
"""
import ctypes
import os

import numpy as np
import torch

from . import dataset_loading as _dl
from .dataset_loading import DataLoader3D

_PAD_MODES = {"constant": 0, "edge": 1}


class DeviceCaseCache:
    """budget_bytes: None keeps every case, 0 keeps none.  ``upload(array) -> device tensor`` is replaceable (tests of the
    bookkeeping run without a GPU).  ``device_inflate``: a case that has no unpacked ``.npy`` is admitted from the shape in its
    ``.npy`` header, before any device work, and its ``data`` member is inflated into HBM by ``deflate.load_npz`` (``loader``
    replaces it in tests: ``loader(raw) -> tensor``) and converted to fp32 there; a member that is not this package's goes
    through ``np.load`` inside ``load_npz`` -- with ``device_inflate="any"`` through ``deflate.inflate_any`` first (zlib-written stage
    folders).  The cases on the device hold the same bits either way."""

    def __init__(self, budget_bytes=None, device="cuda", upload=None, device_inflate=False, loader=None):
        if budget_bytes is not None and budget_bytes < 0:
            raise ValueError("budget_bytes %r: None means no limit, a number of bytes is not negative" % (budget_bytes,))
        self.budget_bytes = None if budget_bytes is None else int(budget_bytes)
        self.device = device
        self._upload = self._to_device if upload is None else upload
        from ... import deflate
        self.foreign = deflate.foreign_of(device_inflate, "DeviceCaseCache: device_inflate")      # None: off
        self.device_inflate = self.foreign is not None
        self._loader = self._inflate_to_device if loader is None else loader
        self.inflated_cases = 0
        self._cases = {}
        self.resident_bytes = 0

    def _to_device(self, array):
        # (a copy: a memory-mapped case is read-only, which torch.from_numpy does not take silently; once per case)
        return torch.from_numpy(np.array(array, dtype=np.float32, order='C')).to(self.device)

    def _inflate_to_device(self, raw):
        from ... import deflate
        return deflate.load_npz(raw, keys=("data",), device=self.device, foreign=self.foreign)["data"]

    def _fetch_inflated(self, path):
        """(case, resident) of a packed case under ``device_inflate``, or None where the host route has to take it: the archive has
        no ``data`` member with a readable header, or the budget has no room"""
        from ... import deflate
        raw = deflate.read_npz_raw(path)
        member = raw.members.get("data")
        if member is None or member.shape is None:
            return None
        nbytes = int(np.prod(member.shape, dtype=np.int64)) * 4
        if self.budget_bytes is not None and self.resident_bytes + nbytes > self.budget_bytes:
            return None
        case = self._loader(raw)
        if case.dtype != torch.float32:
            case = case.to(torch.float32)
        self._cases[path] = case.contiguous()
        self.resident_bytes += nbytes
        self.inflated_cases += 1
        return self._cases[path], True

    def __len__(self):
        return len(self._cases)

    def __contains__(self, path):
        return path in self._cases

    def fetch(self, entry, memmap_mode="r"):
        """(case, resident): the device tensor of a resident case, or the host array (as ``_load_case`` returns it) of one that the
        budget has no room for.  A case met for the first time is admitted when it fits: a case exactly as large as what is left of
        the budget does."""
        path = entry['data_file']
        case = self._cases.get(path)
        if case is not None:
            return case, True
        if self.device_inflate and not os.path.isfile(path[:-4] + ".npy"):
            got = self._fetch_inflated(path)
            if got is not None:
                return got
        host = _dl._load_case(entry, memmap_mode)
        nbytes = int(np.prod(host.shape)) * 4
        if self.budget_bytes is not None and self.resident_bytes + nbytes > self.budget_bytes:
            return host, False
        case = self._upload(host)
        self._cases[path] = case
        self.resident_bytes += nbytes
        return case, True


def device_crop(sources, offsets, num_channels, patch_size, data_mode, data_fill, seg_fill, device):
    """One ``e2e_loader_crop`` launch on the current stream.  sources: per sample a device tensor [C + 1, d, h, w] fp32; offsets: per
    sample the box coordinates of patch voxel (0, 0, 0).  Returns fresh (data [B, C, *patch], seg [B, 1, *patch])."""
    from ..._lib import lib, LoaderRec
    L = lib()
    B = len(sources)
    recs = (LoaderRec * B)()
    for j, (src, off) in enumerate(zip(sources, offsets)):
        if not (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 4
                and src.shape[0] == num_channels + 1):
            raise ValueError("sample %d: the source must be a contiguous fp32 device tensor [%d, d, h, w], got %s %s"
                             % (j, num_channels + 1, src.dtype, tuple(src.shape)))
        recs[j] = LoaderRec(src.data_ptr(), int(src.shape[1]), int(src.shape[2]), int(src.shape[3]),
                            int(off[0]), int(off[1]), int(off[2]))
    pd, ph, pw = (int(v) for v in patch_size)
    data = torch.empty((B, num_channels, pd, ph, pw), dtype=torch.float32, device=device)
    seg = torch.empty((B, 1, pd, ph, pw), dtype=torch.float32, device=device)
    L.loader_crop(ctypes.addressof(recs), B, num_channels, pd, ph, pw, data.data_ptr(), seg.data_ptr(), int(data_mode),
                  float(data_fill), float(seg_fill), torch.cuda.current_stream().cuda_stream)
    return data, seg


class _StagingSet:
    """The page-locked host buffers one batch stages its non-resident samples through, and the event behind their uploads."""

    def __init__(self):
        self.buffers = []
        self.event = None

    def buffer(self, index, numel):
        while len(self.buffers) <= index:
            self.buffers.append(None)
        if self.buffers[index] is None or self.buffers[index].numel() < numel:
            self.buffers[index] = torch.empty(numel, dtype=torch.float32, pin_memory=True)
        return self.buffers[index][:numel]


class ResidentDataLoader3D(DataLoader3D):
    """``DataLoader3D`` whose batches are device tensors cut by one kernel launch out of ``cache``; iterating yields
    {'data', 'seg', 'properties', 'keys'} forever (no 'data_pinned': there is no host batch).  ``crop`` replaces the launch (tests of
    the draw order run without a GPU)."""

    def __init__(self, data, patch_size, final_patch_size, batch_size, has_prev_stage=False,
                 oversample_foreground_percent=0.0, memmap_mode="r", pad_mode="edge", pad_kwargs_data=None,
                 pad_sides=None, pin_memory=None, num_buffers=2, cache=None, crop=None):
        if has_prev_stage:
            raise NotImplementedError("ResidentDataLoader3D: the cascade's previous-stage segmentation is not built; use DataLoader3D")
        if pad_mode not in _PAD_MODES:
            raise NotImplementedError("ResidentDataLoader3D: pad_mode %r; the kernel pads with 'constant' or 'edge'" % (pad_mode,))
        if crop is None and not torch.cuda.is_available():
            raise RuntimeError("ResidentDataLoader3D cuts its batches on the GPU and no GPU is visible; there is no CPU fallback "
                               "(DataLoader3D is the host loader)")
        if cache is None:
            raise ValueError("ResidentDataLoader3D needs a DeviceCaseCache (one is shared by the train and validation loaders)")
        self.cache = cache
        self._crop = crop
        self._staging = [_StagingSet() for _ in range(max(2, num_buffers))]
        self.batches = self.staged_samples = 0
        super().__init__(data, patch_size, final_patch_size, batch_size, False, oversample_foreground_percent, memmap_mode,
                         pad_mode, pad_kwargs_data, pad_sides, pin_memory, num_buffers)
        unknown = set(self.pad_kwargs_data) - {'constant_values'}
        if unknown or pad_mode == "edge" and self.pad_kwargs_data:
            raise NotImplementedError("ResidentDataLoader3D: pad_kwargs_data %r" % (dict(self.pad_kwargs_data),))
        self._data_fill = float(self.pad_kwargs_data.get('constant_values', 0))

    def _allocate_buffers(self, pin_memory, num_buffers):
        self._buffers, self._uploaded, self._turn, self._last = [], [], 0, None

    def mark_uploaded(self, event):
        pass

    def _stage(self, staging, index, host, bb):
        """Upload the part of the host case that the patch at bb covers (at least one plane per axis, so that 'edge' finds its
        border); returns (device box, its corner in case coordinates)."""
        ps = self.patch_size
        shape = host.shape[1:]
        lo = [min(max(int(bb[d]), 0), shape[d] - 1) for d in range(3)]
        hi = [max(min(int(bb[d]) + int(ps[d]), shape[d]), lo[d] + 1) for d in range(3)]
        ext = [hi[d] - lo[d] for d in range(3)]
        pinned = staging.buffer(index, host.shape[0] * ext[0] * ext[1] * ext[2]).view(host.shape[0], *ext)
        pinned.numpy()[...] = host[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        return pinned.to(self.cache.device, non_blocking=True), lo

    def generate_train_batch(self):
        resident = []

        def open_case(entry):
            case, is_resident = self.cache.fetch(entry, self.memmap_mode)
            resident.append(is_resident)
            return case
        selected_keys, plan = self.draw_batch(open_case)
        staging = self._staging[self._turn]
        self._turn = (self._turn + 1) % len(self._staging)
        sources, offsets, staged = [], [], 0
        for j, (properties, case, _, bb) in enumerate(plan):
            if resident[j]:
                sources.append(case)
                offsets.append([int(v) for v in bb])
                continue
            if staged == 0 and staging.event is not None:       # the uploads of two batches ago may still read these buffers
                staging.event.synchronize()
                staging.event = None
            box, lo = self._stage(staging, staged, case, bb)
            staged += 1
            sources.append(box)
            offsets.append([int(bb[d]) - lo[d] for d in range(3)])
        if staged:
            staging.event = torch.cuda.Event()
            staging.event.record(torch.cuda.current_stream())
        crop = device_crop if self._crop is None else self._crop
        data, seg = crop(sources, offsets, self.num_channels, self.patch_size, _PAD_MODES[self.pad_mode], self._data_fill, -1.0,
                         self.cache.device)
        self.batches += 1
        self.staged_samples += staged
        return {'data': data, 'seg': seg, 'properties': [p[0] for p in plan], 'keys': selected_keys}

    def residency_report(self):
        """the trainer's log line"""
        return ("resident data: %d cases (%.3f GiB) on the device, %.2f samples staged per batch over %d batches"
                % (len(self.cache), self.cache.resident_bytes / 2.0 ** 30, self.staged_samples / max(1, self.batches), self.batches))
