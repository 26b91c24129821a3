"""Drop-in for jdacs-ms/models/seg_dff.py: the same NMF / SegDFF as jdacs (mvs_amd.jdacs.models.seg_dff), re-exported."""
from ...jdacs.models.seg_dff import MAX_ATTEMPTS, NMF, SegDFF, initial_factors  # noqa: F401
