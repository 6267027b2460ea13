"""The host half of the intensity statistics of the dataset fingerprint (reference e2enet/experiment_planning/DatasetAnalyzer.py:168-179,
``_compute_stats``): which order statistics of a sample of ``n`` values the seven numbers need, and how those, the extrema and two
fp64 sums become median, mean, sd, min, max and the two percentiles.  numpy only: no device and no library is needed to import or
call this module.  The device half (csrc/fingerprint.hip) supplies the order statistics without sorting and the sums.

The rule: the median is the middle element or the mean of the two middle ones; a percentile is the linear
interpolation between the two order statistics around the virtual index ``(n - 1) q / 100``, with numpy's own fp64 arithmetic for
that index and for the interpolation; mean and population sd come from fp64 sums.  Everything is formed in fp64 and rounded once to
fp32, the type numpy returns for fp32 input."""
import numpy as np

PERCENTILES = (99.5, 0.5)            # reference :177-178, in the order _compute_stats returns them
STAT_NAMES = ('median', 'mean', 'sd', 'mn', 'mx', 'percentile_99_5', 'percentile_00_5')
MAX_RANKS = 8                        # one call of the device select serves this many; the seven numbers need at most 6


def median_ranks(n):
    """positions in the sorted sample of the one or two middle elements"""
    n = int(n)
    return (n - 1) // 2, n // 2


def percentile_ranks(n, q):
    """``(lo, hi, t)``: the percentile is ``s[lo] + t (s[hi] - s[lo])``.  numpy's 'linear' method in fp64: the virtual index is
    ``(n - 1) * (q / 100)``, ``lo`` its floor, ``hi`` the next position (the last one at most)"""
    n = int(n)
    virtual = np.float64(n - 1) * (np.float64(q) / np.float64(100))
    lo = int(np.floor(virtual))
    lo = min(max(lo, 0), n - 1)
    return lo, min(lo + 1, n - 1), np.float64(virtual - lo)


def requested_ranks(n):
    """the ascending, distinct positions of the sorted sample that ``stats_from_order_statistics`` reads for ``n >= 1`` values"""
    ranks = set(median_ranks(n))
    for q in PERCENTILES:
        lo, hi, _ = percentile_ranks(n, q)
        ranks.update((lo, hi))
    ranks = sorted(ranks)
    assert len(ranks) <= MAX_RANKS
    return ranks


def _lerp(a, b, t):
    """numpy's _lerp (lib/_function_base_impl.py) on fp64 scalars"""
    with np.errstate(invalid='ignore', over='ignore'):
        a, b, t = np.float64(a), np.float64(b), np.float64(t)
        diff = b - a
        return b - diff * (1 - t) if t >= 0.5 else a + diff * t


def all_nan():
    """seven ``np.nan``, the reference's answer for an empty sample (:170-171)"""
    return (np.nan,) * 7


def stats_from_order_statistics(n, num_nan, minimum, maximum, total, sq_dev, order):
    """``(median, mean, sd, mn, mx, percentile_99_5, percentile_00_5)`` as ``np.float32`` of a sample of ``n`` fp32 values.
    ``order[r]``: the value at position ``r`` of the sorted sample for every ``r`` in ``requested_ranks(n)``; ``total``: the fp64
    sum; ``sq_dev``: the fp64 sum of ``(x - total / n)**2``.  An empty sample gives seven ``np.nan``; a sample with a NaN gives seven
    fp32 NaN, what every one of numpy's seven calls returns for it."""
    n = int(n)
    if n == 0:
        return all_nan()
    if num_nan:
        return (np.float32(np.nan),) * 7
    with np.errstate(invalid='ignore', over='ignore'):
        lo, hi = median_ranks(n)
        median = np.float32((np.float64(order[lo]) + np.float64(order[hi])) / 2)
        mean = np.float32(np.float64(total) / n)
        sd = np.float32(np.sqrt(np.float64(sq_dev) / n))
        pct = []
        for q in PERCENTILES:
            lo, hi, t = percentile_ranks(n, q)
            pct.append(np.float32(_lerp(order[lo], order[hi], t)))
    return median, mean, sd, np.float32(minimum), np.float32(maximum), pct[0], pct[1]


def stats_of_sorted(sorted_values):
    """the same from a sorted fp32 array on the host (the restatement of the device path that the tests and the DESIGN section 9 measurement use)"""
    s = np.asarray(sorted_values, dtype=np.float32)
    n = s.size
    if n == 0:
        return all_nan()
    x = s.astype(np.float64)
    num_nan = int(np.isnan(x).sum())
    with np.errstate(invalid='ignore', over='ignore'):
        total = x.sum()
        sq_dev = ((x - total / n) ** 2).sum()
    return stats_from_order_statistics(n, num_nan, s[0], s[-1], total, sq_dev, {r: s[r] for r in requested_ranks(n)})
