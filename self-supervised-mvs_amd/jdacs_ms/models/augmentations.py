"""Drop-in for the two functions of jdacs-ms/models/augmentations.py that train.py calls (:16-39): the same as jdacs, re-exported."""
from ...jdacs.models.augmentations import aug_loss, random_image_mask  # noqa: F401
