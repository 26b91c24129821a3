"""Drop-in for jdacs-ms/losses/unsup_seg_loss.py:20-89 (compute_seg_loss, UnSupSegLoss -- the class train.py:97 builds): the same
computation as jdacs (mvs_amd.jdacs.losses.unsup_seg_loss), re-exported.  UnSupSegLossAcc (:92) is not called by train.py and is
not provided."""
from ...jdacs.losses.unsup_seg_loss import UnSupSegLoss, compute_seg_loss  # noqa: F401
