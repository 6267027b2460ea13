"""Host yardstick of the ensembling step (csrc/ensemble.hip, inference/ensemble_predictions.py): numpy itself, making the calls the
reference makes.  The reference's merge_files cannot run here (SimpleITK, batchgenerators), so its array expressions are restated:
  * ``np.vstack`` of the volumes with a leading axis, ``np.mean`` over it (ensemble_predictions.py:28-30);
  * ``.astype(np.float16)`` of the transposed fp32 softmax (segmentation_export.py:118, predict.py:298-301);
  * ``argmax(0)``, or one pass per region ``final[mean[i] > 0.5] = c`` (segmentation_export.py:124-130);
  * the uint8 volume of the original size with the result in the crop box, the box clipped to that size (:132-142);
  * with a post-processing decision, tests/cc_oracle.py on that volume (what apply_postprocessing_to_folder does per file).
``sequential_mean`` is the rule the kernel implements, stated without np.mean; tests/test_ensemble_cpu.py holds the two together."""
import numpy as np


def mean_softmax(softmaxes):
    softmax = [np.asarray(s)[None] for s in softmaxes]
    softmax = np.vstack(softmax)
    return np.mean(softmax, 0)


def mean_softmax_tuple(a, b):
    """the other form the reference uses for two models (evaluation/model_selection/ensemble.py): np.mean((a, b), 0)"""
    return np.mean((a, b), 0)


def sequential_mean(softmaxes):
    """fp32 sum in source order, one fp32 division by the number of sources, one rounding to fp16"""
    acc = np.asarray(softmaxes[0]).astype(np.float32)
    for s in softmaxes[1:]:
        acc = acc + np.asarray(s).astype(np.float32)
    return (acc / np.float32(len(softmaxes))).astype(np.float16)


def softmax_to_f16(softmax, transpose_backward=None):
    tb = [0, 1, 2] if transpose_backward is None else list(transpose_backward)
    return np.ascontiguousarray(softmax.transpose([0] + [i + 1 for i in tb]).astype(np.float16))


def labels(mean, regions_class_order=None):
    if regions_class_order is None:
        return mean.argmax(0)
    final = np.zeros(mean.shape[1:])
    for i, c in enumerate(regions_class_order):
        final[mean[i] > 0.5] = c
    return final


def place(seg, properties):
    bbox = properties.get('crop_bbox')
    if bbox is None:
        return seg.astype(np.uint8)
    full = properties.get('original_size_of_raw_data')
    out = np.zeros([int(v) for v in full], dtype=np.uint8)
    lo = [int(bbox[c][0]) for c in range(3)]
    hi = [int(np.min((lo[c] + seg.shape[c], full[c]))) for c in range(3)]
    out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = seg[:hi[0] - lo[0], :hi[1] - lo[1], :hi[2] - lo[2]]
    return out


def merge_softmax(softmaxes, properties, regions_class_order=None, postprocessing=None, return_mean=False, return_raw=False):
    """the interface of inference.ensemble_predictions.merge_softmax on host arrays"""
    from tests import cc_oracle
    mean = mean_softmax(softmaxes)
    assert mean.dtype == np.float16
    assert tuple(mean.shape[1:]) == tuple(int(v) for v in properties['size_after_cropping']), "the oracle does not resample"
    raw = place(labels(mean, regions_class_order), properties)
    seg = raw
    if postprocessing is not None:
        vpv = float(np.prod(properties['itk_spacing'], dtype=np.float64))
        seg = cc_oracle.remove_all_but_the_largest_connected_component(raw.copy(), postprocessing[0], vpv, postprocessing[1])[0]
    out = (seg,) + ((raw,) if return_raw else ()) + ((mean,) if return_mean else ())
    return out[0] if len(out) == 1 else out


def near_uniform(n_sources, k, shape, seed, scale=0.05):
    """N fp16 softmax volumes of ``scale * randn`` logits: class probabilities a few fp16 steps apart, so that the fp16 means tie and
    their order differs from that of the fp32 means"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n_sources):
        z = (scale * rng.randn(k, *shape)).astype(np.float32)
        e = np.exp(z - z.max(0, keepdims=True))
        out.append((e / e.sum(0, keepdims=True)).astype(np.float16))
    return out


def tie_and_flip_counts(softmaxes):
    """(voxels whose two largest fp16 means are equal, voxels whose label differs from the label of the fp32 mean)"""
    m16 = mean_softmax(softmaxes)
    acc = np.asarray(softmaxes[0]).astype(np.float32)
    for s in softmaxes[1:]:
        acc = acc + np.asarray(s).astype(np.float32)
    m32 = acc / np.float32(len(softmaxes))
    top = np.sort(m16, 0)
    return int((top[-1] == top[-2]).sum()), int((m16.argmax(0) != m32.argmax(0)).sum())


def properties(size, original=None, offset=(0, 0, 0), spacing=(0.7, 0.8, 2.5)):
    """the entries of a case's properties the export reads"""
    original = list(size) if original is None else list(original)
    return {'size_after_cropping': np.array(size), 'original_size_of_raw_data': np.array(original),
            'crop_bbox': [[int(o), int(o) + int(s)] for o, s in zip(offset, size)], 'itk_spacing': tuple(spacing)}
