"""The pooling and kernel-size layout of a U-Net for a patch and a spacing: the reference's
e2enet/experiment_planning/common_utils.py:50-155, 232-275 under the reference's names, host integer and fp64 arithmetic.

  get_pool_and_conv_props              :89-154   pools by spacing: an axis is pooled while it is within a factor 2 of the finest one
  get_pool_and_conv_props_poolLateV2   :50-86    pools as late as possible: the axis with fewer poolings skips the first ones
  get_shape_must_be_divisible_by       :232-233
  pad_shape                            :236-254
  get_network_numpool                  :257-260

Every function returns what the reference returns, type for type (lists of Python ints, ``np.int64`` where numpy made the number,
``np.ndarray`` for the padded patch): the plans file holds these objects as they come.  ``split_4d_nifti`` is not part of this
package."""
from copy import deepcopy

import numpy as np


def get_shape_must_be_divisible_by(net_numpool_per_axis):
    """2 ** poolings, per axis"""
    return 2 ** np.array(net_numpool_per_axis)


def pad_shape(shape, must_be_divisible_by):
    """``shape`` rounded up, axis by axis, to a multiple of ``must_be_divisible_by`` (one number or one per axis); an int array"""
    if isinstance(must_be_divisible_by, (tuple, list, np.ndarray)):
        assert len(must_be_divisible_by) == len(shape)
    else:
        must_be_divisible_by = [must_be_divisible_by] * len(shape)
    padded = []
    for s, m in zip(shape, must_be_divisible_by):
        rest = s % m
        padded.append(s if rest == 0 else s + m - rest)
    return np.array(padded).astype(int)


def get_network_numpool(patch_size, maxpool_cap=999, min_feature_map_size=4):
    """poolings per axis that leave at least ``min_feature_map_size`` voxels: floor(log2(edge / min)), capped"""
    per_axis = np.floor([np.log(edge / min_feature_map_size) / np.log(2) for edge in patch_size]).astype(int)
    return [min(n, maxpool_cap) for n in per_axis]


def get_pool_and_conv_props_poolLateV2(patch_size, min_feature_map_size, max_numpool, spacing):
    """``(num_pool_per_axis, pool_op_kernel_sizes, conv_kernel_sizes, padded patch_size, must_be_divisible_by)``.  The number of
    poolings of an axis comes from its edge alone; an axis with fewer than the deepest one sits out the first stages.  A stage's
    convolution is 3 along an axis once that axis's spacing (doubled by every pooling so far) exceeds half the coarsest original
    spacing, 1 before that -- unless every axis is there, then 3 throughout."""
    reach = max(deepcopy(spacing))
    dim = len(patch_size)
    num_pool_per_axis = get_network_numpool(patch_size, max_numpool, min_feature_map_size)
    depth = max(num_pool_per_axis)
    pool_op_kernel_sizes, conv_kernel_sizes = [], []
    current_spacing = spacing
    for stage in range(depth):
        reached = [current_spacing[a] / reach > 0.5 for a in range(dim)]
        pool = [2 if num_pool_per_axis[a] + stage >= depth else 1 for a in range(dim)]
        conv_kernel_sizes.append([3] * dim if all(reached) else [1 if reached[a] else 3 for a in range(dim)])
        pool_op_kernel_sizes.append(pool)
        current_spacing = [s * p for s, p in zip(current_spacing, pool)]
    conv_kernel_sizes.append([3] * dim)                        # the bottleneck
    must_be_divisible_by = get_shape_must_be_divisible_by(num_pool_per_axis)
    return num_pool_per_axis, pool_op_kernel_sizes, conv_kernel_sizes, pad_shape(patch_size, must_be_divisible_by), must_be_divisible_by


def get_pool_and_conv_props(spacing, patch_size, min_feature_map_size, max_numpool):
    """The same five values, pooling by spacing.  Stage by stage: the axes whose spacing is below twice the finest one are pooled
    (spacing doubled, edge halved and rounded up) as long as their edge is at least ``2 * min_feature_map_size`` and they have fewer
    than ``max_numpool`` poolings; the stage's convolution is 3 along the largest group of axes whose spacings are within a factor 2
    of each other (the first such group in axis order), 1 elsewhere.  It ends when no axis can be pooled."""
    dim = len(spacing)
    current_spacing = deepcopy(list(spacing))
    current_size = deepcopy(list(patch_size))
    pool_op_kernel_sizes, conv_kernel_sizes = [], []
    num_pool_per_axis = [0] * dim
    while True:
        finest = min(current_spacing)
        candidates = [a for a in range(dim) if current_spacing[a] / finest < 2]
        group = []
        for a in range(dim):
            mine = current_spacing[a]
            close = [b for b in range(dim) if current_spacing[b] / mine < 2 and mine / current_spacing[b] < 2]
            if len(close) > len(group):
                group = close
        conv = [3 if a in group else 1 for a in range(dim)]
        candidates = [a for a in candidates if current_size[a] >= 2 * min_feature_map_size]
        candidates = [a for a in candidates if num_pool_per_axis[a] < max_numpool]
        if not candidates:
            break
        pool = [1] * dim
        for a in candidates:
            pool[a] = 2
            num_pool_per_axis[a] += 1
            current_spacing[a] *= 2
            current_size[a] = np.ceil(current_size[a] / 2)
        pool_op_kernel_sizes.append(pool)
        conv_kernel_sizes.append(conv)
    must_be_divisible_by = get_shape_must_be_divisible_by(num_pool_per_axis)
    patch_size = pad_shape(patch_size, must_be_divisible_by)
    conv_kernel_sizes.append([3] * dim)                        # the bottleneck
    return num_pool_per_axis, pool_op_kernel_sizes, conv_kernel_sizes, patch_size, must_be_divisible_by
