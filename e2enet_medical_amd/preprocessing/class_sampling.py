"""The host half of the class-location sampling (reference e2enet/preprocessing/preprocessing.py:343-361): how many voxels of a class
are kept and which ones, as ranks into ``np.argwhere(seg == c)``.  numpy only: no device and no library is needed to import or call
this module.  The device half (csrc/class_select.hip) turns ranks into coordinates without listing a class's voxels."""
import numpy as np

NUM_SAMPLES = 10000                  # reference :346
MIN_PERCENT_COVERAGE = 0.01          # reference :347: at least 1% of a class's voxels
SEED = 1234                          # reference :348


def target_num_samples(n, num_samples=NUM_SAMPLES, min_percent_coverage=MIN_PERCENT_COVERAGE):
    """Reference :355-356: ``max(min(num_samples, n), ceil(n * min_percent_coverage))``; 0 for an empty class"""
    n = int(n)
    if n == 0:
        return 0
    return max(min(int(num_samples), n), int(np.ceil(n * min_percent_coverage)))


def draw_ranks(counts, num_samples=NUM_SAMPLES, min_percent_coverage=MIN_PERCENT_COVERAGE, seed=SEED):
    """One entry per count, in order: the int64 rows of ``np.argwhere(seg == c)`` the reference keeps for a class with that many
    voxels, in the order it keeps them.  One ``RandomState(seed)`` serves the classes in turn with the reference's own call,
    ``choice(n, t, replace=False)``; an empty class gets ``[]`` and consumes no random numbers."""
    rndst = np.random.RandomState(seed)
    drawn = []
    for n in counts:
        n = int(n)
        if n == 0:
            drawn.append([])
            continue
        drawn.append(rndst.choice(n, target_num_samples(n, num_samples, min_percent_coverage), replace=False).astype(np.int64))
    return drawn


def draw_class_ranks(all_classes, counts, num_samples=NUM_SAMPLES, min_percent_coverage=MIN_PERCENT_COVERAGE, seed=SEED):
    """``{c: ranks}`` in the order of ``all_classes`` (not sorted), given only ``counts[i] = (seg == all_classes[i]).sum()``:
    ``np.argwhere(seg == c)[ranks]`` is the reference's ``class_locations[c]``"""
    assert len(all_classes) == len(counts), "one count per class"
    return dict(zip(all_classes, draw_ranks(counts, num_samples, min_percent_coverage, seed)))


def sort_ranks(ranks):
    """``(sorted ranks, slots)`` of one class's draw: ``slots[p]`` is the place of ``sorted[p]`` in the draw"""
    ranks = np.asarray(ranks, dtype=np.int64)
    slots = np.argsort(ranks, kind="stable").astype(np.int64)
    return ranks[slots], slots
