"""The cascade's transforms on the device (kernels: csrc/cascade.hip).

Mirrors reference e2enet/training/data_augmentation/pyramid_augmentations.py:23-136 -- ``MoveSegAsOneHotToData``,
``ApplyRandomBinaryOperatorTransform`` and ``RemoveRandomConnectedComponentFromOneHotEncodingTransform`` with the reference's
constructor arguments -- restated for a dict of DEVICE tensors.  The reference runs scikit-image's ``ball``, ``binary_dilation`` /
``erosion`` / ``closing`` / ``opening`` and ``label`` on the host for every one-hot channel of the previous stage's segmentation;
here the channel is bit-packed once, a morphology pass ORs shifted words over the footprint's x-runs, and the components come from the
union-find the post-processing uses, with full (26-neighbour) connectivity.

Each transform splits into ``draw(rs, B)`` -- every random number, from a ``numpy.random.RandomState``, independent of the data --
and ``apply(data, draws)``, a pure function of its arguments.  The three data-dependent choices of the component removal (which
component, whether to fill, with which other channel) are three uniforms mapped by ``floor(u * n)``; the reference asks
``np.random.choice`` only when a component qualifies, so its call stream differs.

scikit-image is absent: ``ball`` restates its rule and tests/test_cascade_cpu.py pins it to the literal expression; the morphology
is tested against ``scipy.ndimage`` with the border values scikit-image passes.
"""
import numpy as np
import torch

from ..._lib import lib

DILATION, EROSION, CLOSING, OPENING = 0, 1, 2, 3
OPERATION_NAMES = ("binary_dilation", "binary_erosion", "binary_closing", "binary_opening")
# (reflect, complement) of the passes of an operation: erosion is the complemented dilation of the complement by the reflected footprint
_PASSES = {DILATION: ((0, 0),), EROSION: ((1, 1),), CLOSING: ((0, 0), (1, 1)), OPENING: ((1, 1), (0, 0))}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def ball(radius):
    """skimage.morphology.ball (0.19): ``n = 2 r + 1``, ``Z, Y, X = np.mgrid[-r:r:n*1j, -r:r:n*1j, -r:r:n*1j]``,
    ``X**2 + Y**2 + Z**2 <= r * r``.  A float radius gives int(2 r + 1) points per axis, evenly spaced over [-r, r] with mgrid's
    arithmetic (index * step + start: the last point is not pinned to r)."""
    r = radius
    n = int(2 * r + 1)
    ax = np.arange(n, dtype=np.float64)
    if n > 1:
        ax = ax * ((r - (-r)) / float(n - 1)) + (-r)
    else:
        ax = ax + (-r)
    s = ax ** 2
    return (s[None, None, :] + s[None, :, None] + s[:, None, None]) <= r * r


def run_table(footprint):
    """(table int32 [n, 4], N): one row (oz, oy, x_lo, x_hi) per maximal x-run of every (z, y) row of a cubic footprint, offsets
    from its origin N // 2.  A row with a gap yields two runs with the same (oz, oy); e2e_morph_pass refuses such a table."""
    fp = np.asarray(footprint) != 0
    assert fp.ndim == 3 and fp.shape[0] == fp.shape[1] == fp.shape[2], "a cubic 3-D footprint"
    n = fp.shape[0]
    c = n // 2
    rows = []
    for z in range(n):
        for y in range(n):
            line = np.concatenate(([False], fp[z, y], [False]))
            edges = np.flatnonzero(line[1:] != line[:-1])           # run starts and (one past) ends, alternating
            for lo, hi in zip(edges[0::2], edges[1::2]):
                rows.append((z - c, y - c, int(lo) - c, int(hi) - 1 - c))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4), n


def _i32(values):
    return np.ascontiguousarray(values, dtype=np.int32)


def seg_onehot(seg: torch.Tensor, channel: int, labels, out: torch.Tensor, first_channel: int):
    """out[:, first_channel + l] = (seg[:, channel] == labels[l]) on the device"""
    assert seg.is_cuda and seg.dtype == torch.float32 and seg.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32
    lab = _i32(labels)
    lib().seg_onehot(seg.data_ptr(), out.data_ptr(), lab.ctypes.data, len(lab), seg.shape[0], seg.shape[1], int(channel), out.shape[1],
                     int(first_channel), int(np.prod(seg.shape[2:])), _stream())
    return out


def binary_operation(sample: torch.Tensor, channel: int, operation: int, footprint, others=(), scratch=None):
    """One of the four operations, in place, on ``sample[channel]`` of a contiguous device sample [C, D, H, W] (values != 0 are set);
    where a voxel was added the ``others`` channels are set to 0.  ``footprint``: a cubic array, or its (table, N)."""
    assert sample.is_cuda and sample.dtype == torch.float32 and sample.is_contiguous() and sample.dim() == 4
    L = lib()
    C, D, H, W = (int(v) for v in sample.shape)
    table, n = footprint if isinstance(footprint, tuple) else run_table(footprint)
    table = _i32(table)
    words = L.morph_bits_words(D, H, W)
    if scratch is None or scratch.numel() < 2 * words:
        scratch = torch.empty(2 * words, dtype=torch.int64, device=sample.device)
    src, dst = scratch[:words], scratch[words:2 * words]
    channel = int(channel) % C
    L.morph_pack(sample[channel].data_ptr(), src.data_ptr(), D, H, W, _stream())
    for reflect, complement in _PASSES[int(operation)]:
        L.morph_pass(src.data_ptr(), dst.data_ptr(), D, H, W, table.ctypes.data, len(table), n, reflect, complement, _stream())
        src, dst = dst, src
    oth = _i32([int(o) % C for o in others])
    L.morph_unpack(src.data_ptr(), sample.data_ptr(), C, channel, oth.ctypes.data, len(oth), D, H, W, _stream())
    return scratch


def remove_component(sample: torch.Tensor, channel: int, threshold: float, u: float, fill_channel=None, ws=None, result=None):
    """Of the 26-connected components of ``sample[channel]`` with size < threshold, in label order, number floor(u * count) is
    cleared and, with ``fill_channel``, set in that channel.  Returns (ws, result): result is a device int64[4] -- components,
    eligible components, size of the removed one, give-up word -- read only by tests and logging."""
    assert sample.is_cuda and sample.dtype == torch.float32 and sample.is_contiguous() and sample.dim() == 4
    L = lib()
    C, D, H, W = (int(v) for v in sample.shape)
    need = (L.rcc_ws_bytes(D, H, W) + 7) // 8
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.int64, device=sample.device)
    if result is None:
        result = torch.empty(4, dtype=torch.int64, device=sample.device)
    fill = sample[int(fill_channel) % C].data_ptr() if fill_channel is not None else None
    L.rcc_remove(sample[int(channel) % C].data_ptr(), fill, D, H, W, float(threshold), float(u), ws.data_ptr(), result.data_ptr(), _stream())
    return ws, result


class MoveSegAsOneHotToData:
    """reference :71-93: ``seg[:, channel_id]`` becomes len(all_seg_labels) one-hot channels behind the data channels and leaves seg."""

    def __init__(self, channel_id, all_seg_labels, key_origin="seg", key_target="data", remove_from_origin=True):
        self.remove_from_origin = remove_from_origin
        self.all_seg_labels = all_seg_labels
        self.key_target = key_target
        self.key_origin = key_origin
        self.channel_id = channel_id

    def apply(self, data: torch.Tensor, seg: torch.Tensor):
        n_data, n_lab = int(data.shape[1]), len(self.all_seg_labels)
        out = torch.empty((data.shape[0], n_data + n_lab) + tuple(data.shape[2:]), dtype=torch.float32, device=data.device)
        out[:, :n_data].copy_(data)
        seg_onehot(seg.contiguous(), self.channel_id, self.all_seg_labels, out, n_data)
        if self.remove_from_origin:
            seg = seg[:, [i for i in range(seg.shape[1]) if i != self.channel_id]].contiguous()
        return out, seg

    def __call__(self, **data_dict):
        data_dict[self.key_target], data_dict[self.key_origin] = self.apply(data_dict[self.key_target], data_dict[self.key_origin])
        return data_dict


class ApplyRandomBinaryOperatorTransform:
    """reference :96-136.  ``any_of_these``: operation codes out of (DILATION, EROSION, CLOSING, OPENING)."""

    def __init__(self, channel_idx, p_per_sample=0.3, any_of_these=(DILATION, EROSION, CLOSING, OPENING), key="data", strel_size=(1, 10),
                 p_per_label=1, rs=None):
        self.p_per_label = p_per_label
        self.strel_size = strel_size
        self.key = key
        self.any_of_these = tuple(any_of_these)
        self.p_per_sample = p_per_sample
        assert not isinstance(channel_idx, tuple), "channel_idx is an int or a list"
        if not isinstance(channel_idx, list):
            channel_idx = [channel_idx]
        self.channel_idx = channel_idx
        self.rs = rs

    def draw(self, rs, B):
        """Per sample: uniform() < p_per_sample, a shuffle of the channel list; per channel in that order: uniform() < p_per_label,
        the operation as randint(len(any_of_these)), the radius as uniform(*strel_size).  Returns per sample the list of
        (channel, operation, radius, other channels) in execution order."""
        out = []
        for _ in range(B):
            todo = []
            if rs.uniform() < self.p_per_sample:
                ch = list(self.channel_idx)
                rs.shuffle(ch)
                for c in ch:
                    if rs.uniform() < self.p_per_label:
                        op = self.any_of_these[int(rs.randint(len(self.any_of_these)))]
                        radius = float(rs.uniform(*self.strel_size))
                        todo.append((c, op, radius, [i for i in ch if i != c]))
            out.append(todo)
        return out

    def apply(self, data: torch.Tensor, draws):
        scratch = None
        for b, todo in enumerate(draws):
            for c, op, radius, others in todo:
                scratch = binary_operation(data[b], c, op, ball(radius), others, scratch)
        return data

    def __call__(self, **data_dict):
        data = data_dict[self.key]
        data_dict[self.key] = self.apply(data, self.draw(self.rs if self.rs is not None else np.random, data.shape[0]))
        return data_dict


class RemoveRandomConnectedComponentFromOneHotEncodingTransform:
    """reference :23-68.  A component qualifies when its size is below ``num_voxels * dont_do_if_covers_more_than_X_percent``."""

    def __init__(self, channel_idx, key="data", p_per_sample=0.2, fill_with_other_class_p=0.25,
                 dont_do_if_covers_more_than_X_percent=0.25, p_per_label=1, rs=None):
        self.p_per_label = p_per_label
        self.dont_do_if_covers_more_than_X_percent = dont_do_if_covers_more_than_X_percent
        self.fill_with_other_class_p = fill_with_other_class_p
        self.p_per_sample = p_per_sample
        self.key = key
        if not isinstance(channel_idx, (list, tuple)):
            channel_idx = [channel_idx]
        self.channel_idx = channel_idx
        self.rs = rs
        self.last_results = None        # device int64 [n, 4] of the last apply: one row per labelled channel (tests, logging)

    def draw(self, rs, B):
        """Per sample: uniform() < p_per_sample; per channel: uniform() < p_per_label and then three uniforms -- which component,
        whether to fill, with which other channel.  Returns per sample the list of (channel, u_component, u_fill, u_other)."""
        out = []
        for _ in range(B):
            todo = []
            if rs.uniform() < self.p_per_sample:
                for c in self.channel_idx:
                    if rs.uniform() < self.p_per_label:
                        todo.append((c, float(rs.uniform()), float(rs.uniform()), float(rs.uniform())))
            out.append(todo)
        return out

    def apply(self, data: torch.Tensor, draws):
        num_voxels = int(np.prod(data.shape[2:]))
        threshold = float(num_voxels * self.dont_do_if_covers_more_than_X_percent)
        self.last_results = None
        if threshold <= 1:                  # a component has at least one voxel: none is smaller than that (the trainer's defaults: 0.0)
            return data
        n = sum(len(t) for t in draws)
        if n == 0:
            return data
        results = torch.empty((n, 4), dtype=torch.int64, device=data.device)
        ws, k = None, 0
        for b, todo in enumerate(draws):
            for c, u_comp, u_fill, u_other in todo:
                other_ch = [i for i in self.channel_idx if i != c]
                fill = None
                if u_fill < self.fill_with_other_class_p and len(other_ch) > 0:
                    fill = other_ch[min(int(np.floor(u_other * len(other_ch))), len(other_ch) - 1)]
                ws, _ = remove_component(data[b], c, threshold, u_comp, fill, ws, results[k])
                k += 1
        self.last_results = results
        return data

    def __call__(self, **data_dict):
        data = data_dict[self.key]
        data_dict[self.key] = self.apply(data, self.draw(self.rs if self.rs is not None else np.random, data.shape[0]))
        return data_dict
