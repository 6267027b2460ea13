"""The stock U-Net of the reference (e2enet/network_architecture/generic_UNet.py:201-483, ``Tconv='ori'``) as far as the experiment
planner needs it: the class constants (:202-216) and the activation-volume estimate ``compute_approx_vram_consumption`` (:445-483) by
which the planner sizes patches and batches.  The estimate is the stock network's on purpose, not shiftConvPP's: the plans file must
be the one the reference writes.  The network itself is not built here: constructing it raises what ``Tconv='ori'`` raises in the
trainer."""
import numpy as np


class Generic_UNet(object):
    DEFAULT_BATCH_SIZE_3D = 2
    DEFAULT_PATCH_SIZE_3D = (64, 192, 160)
    SPACING_FACTOR_BETWEEN_STAGES = 2
    BASE_NUM_FEATURES_3D = 30
    MAX_NUMPOOL_3D = 999
    MAX_NUM_FILTERS_3D = 320

    DEFAULT_PATCH_SIZE_2D = (256, 256)
    BASE_NUM_FEATURES_2D = 30
    DEFAULT_BATCH_SIZE_2D = 50
    MAX_NUMPOOL_2D = 999
    MAX_FILTERS_2D = 480

    use_this_for_batch_size_computation_2D = 19739648
    use_this_for_batch_size_computation_3D = 520000000

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("the MI355X engine implements Tconv='shiftConvPP' and its ablations 'shiftConvPP_313', "
                                  "'shiftConvPP_331', 'shiftConvPP_noshift', 'shiftConvPP_nodff' (got %r)" % ('ori',))

    @staticmethod
    def compute_approx_vram_consumption(patch_size, num_pool_per_axis, base_num_features, max_num_features, num_modalities,
                                        num_classes, pool_op_kernel_sizes, deep_supervision=False, conv_per_stage=2):
        """A number the activation memory of the stock U-Net is roughly proportional to (``np.int64``): voxels times feature maps,
        summed over the full-resolution stage (``2 * conv_per_stage + 1`` blocks of ``base_num_features``, the input and the output)
        and every pooled stage (features doubled up to ``max_num_features``; the edges divided by the stage's pooling and truncated;
        ``2 * conv_per_stage + 1`` blocks, ``conv_per_stage`` in the bottleneck), plus the deep-supervision outputs when asked."""
        if not isinstance(num_pool_per_axis, np.ndarray):
            num_pool_per_axis = np.array(num_pool_per_axis)
        stages = len(pool_op_kernel_sizes)
        blocks = conv_per_stage * 2 + 1
        map_size = np.array(patch_size)
        voxels = np.prod(map_size, dtype=np.int64)
        total = np.int64(blocks * voxels * base_num_features + num_modalities * voxels + num_classes * voxels)
        num_feat = base_num_features
        for s in range(stages):
            for a in range(len(num_pool_per_axis)):
                map_size[a] = map_size[a] / pool_op_kernel_sizes[s][a]             # (an integer array: the quotient is truncated)
            num_feat = min(num_feat * 2, max_num_features)
            voxels = np.prod(map_size, dtype=np.int64)
            total += (blocks if s < stages - 1 else conv_per_stage) * voxels * num_feat
            if deep_supervision and s < stages - 2:
                total += voxels * num_classes
        return total
