"""Drop-in for jdacs-ms/models/augmentations.py: the two functions train.py calls (:16-39) and the augmentation module with its
transforms: the same as jdacs, re-exported."""
from ...jdacs.models.augmentations import Augmentor, RandomGamma, aug_loss, get_transform, random_image_mask  # noqa: F401
