"""Drop-in names of jdacs-ms/utils.py: the reference keeps the same text in both trees, so these are the jdacs ones
(mvs_amd.jdacs.utils), re-exported.  ``depth_metrics`` / ``DepthMetricsMeter`` serve the block at jdacs-ms/train.py:271-277."""
from ..jdacs.utils import (AbsDepthError_metrics, DepthMetricsMeter, DictAverageMeter, METRIC_KEYS, Thres_metrics,  # noqa: F401
                           compute_metrics_for_each_image, depth_metrics, make_nograd_func, tensor2float, tensor2numpy)
