"""Region targets (reference e2enet/training/data_augmentation/custom_transforms.py:96-123).

A region is a set of integer labels and regions may overlap.  On the device a region is one 32-bit word: bit ``t`` of word
``r`` says "label ``t`` belongs to region ``r``" (``region_words``).  The loss and online-evaluation kernels form the region
targets from the label map through these words on load; ``ConvertSegmentationToRegionsTransform`` writes them out as the
reference's transform does, for callers who want the multi-hot tensor itself.
"""
import torch

from ..._lib import lib

MAX_REGIONS = 32          # KMAX of csrc/loss.hip
MAX_LABEL = 31            # a label is a bit position of a 32-bit word


def region_label_sets(regions):
    """the label tuples of ``regions`` (a dict name -> labels as the reference uses, or a sequence of label tuples), in order"""
    sets = list(regions.values()) if isinstance(regions, dict) else list(regions)
    return [tuple(int(l) for l in (s if isinstance(s, (tuple, list)) else (s,))) for s in sets]


def region_words(regions):
    """tuple of ints, one per region: bit t set = label t belongs to the region.  Labels must lie in [0, 31]."""
    sets = region_label_sets(regions)
    if not 1 <= len(sets) <= MAX_REGIONS:
        raise ValueError("need 1..%d regions, got %d" % (MAX_REGIONS, len(sets)))
    words = []
    for s in sets:
        w = 0
        for l in s:
            if not 0 <= l <= MAX_LABEL:
                raise ValueError("region label %d outside [0, %d]: a region is a 32-bit label set" % (l, MAX_LABEL))
            w |= 1 << l
        words.append(w)
    return tuple(words)


def words_tensor(words, device):
    """device int32 tensor holding the region words' bit patterns (the kernels read them as uint32)"""
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32, device=device)


def seg_to_regions(seg: torch.Tensor, words, channel: int = 0) -> torch.Tensor:
    """label map [B, C, ...] (GPU tensor) -> multi-hot [B, R, ...] float32 0/1 of channel ``channel`` (HIP kernel e2e_seg_to_regions)"""
    if not seg.is_cuda:
        raise RuntimeError("seg_to_regions (MI355X) needs a GPU tensor: there is no CPU fallback")
    lab = seg[:, channel].float().contiguous()
    b = lab.shape[0]
    spatial = lab[0].numel()
    out = torch.empty((b, len(words)) + tuple(lab.shape[1:]), dtype=torch.float32, device=seg.device)
    lib().seg_to_regions(lab.data_ptr(), words_tensor(words, seg.device).data_ptr(), out.data_ptr(), b, len(words), spatial,
                         torch.cuda.current_stream().cuda_stream)
    return out


class ConvertSegmentationToRegionsTransform(object):
    def __init__(self, regions: dict, seg_key: str = "seg", output_key: str = "seg", seg_channel: int = 0):
        """regions: name -> tuple of the labels merged into that region, e.g. {"a": (1, 2), "b": (2,)} gives two regions, one
        covering labels 1 and 2 and the other label 2 only.  ``data_dict[seg_key]`` is a device tensor [B, C, ...], or a list of
        them (deep-supervision scales); the result holds one channel per region."""
        self.seg_channel = seg_channel
        self.output_key = output_key
        self.seg_key = seg_key
        self.regions = regions
        self.words = region_words(regions)

    def __call__(self, **data_dict):
        seg = data_dict.get(self.seg_key)
        if seg is not None:
            if isinstance(seg, (list, tuple)):
                data_dict[self.output_key] = [seg_to_regions(s, self.words, self.seg_channel) for s in seg]
            else:
                data_dict[self.output_key] = seg_to_regions(seg, self.words, self.seg_channel)
        return data_dict
