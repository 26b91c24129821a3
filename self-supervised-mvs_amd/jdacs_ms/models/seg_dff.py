"""Drop-in for jdacs-ms/models/seg_dff.py: the same NMF / SegDFF as jdacs (mvs_amd.jdacs.models.seg_dff), re-exported."""
from ...jdacs.models.seg_dff import (MAX_ATTEMPTS, NMF, VGG19_LAYERS, SegDFF, conv_trunk, initial_factors, trunk_layers,  # noqa: F401
                                     trunk_served, vgg19_trunk)
