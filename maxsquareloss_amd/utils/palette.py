"""The host tables of the prediction images (ops.predict_images, ops.colorize): the Cityscapes colour of
every trainId, and per class count the three tables msl_predict_images reads - class -> labelId, class ->
colour, (confidence bucket, class) -> shaded colour.  Numpy only; no GPU.

A 16- or 13-class model's class k is the k-th entry of synthia_set_16 / synthia_set_13, so it is mapped to
its Cityscapes trainId first: a 16-class "sky" (class 9) is trainId 10, sky-coloured, labelId 23.  (The
reference's decode_labels paints class index k with colour k whatever the class count; for 19 classes the
two are the same.)
"""
import numpy as np

from .preprocess import CITYSCAPES_ID_TO_TRAINID, SET_13, SET_16

# the Cityscapes colours of the 19 trainIds, then black for the ignored label (index -1 / 19)
label_colours = [(128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153),
                 (250, 170, 30), (220, 220, 0), (107, 142, 35), (152, 251, 152), (0, 130, 180), (220, 20, 60),
                 (255, 0, 0), (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32),
                 (0, 0, 0)]

# inspect_decode_labels' splits and brightness ratios (cityscapes_Dataset.py:402-403): the winning
# probability p > SPLITS[b] (first b that holds) is painted at RATIOS[b] of the class colour, black below
SPLITS = (0.9, 0.8, 0.7, 0.5)
RATIOS = (1.0, 0.8, 0.6, 0.3)

TRAINID_TO_ID = {t: i for i, t in CITYSCAPES_ID_TO_TRAINID.items()}


def trainids_of(num_classes):
    """The Cityscapes trainId of each class of a 19-, 16- or 13-class model."""
    sets = {19: list(range(19)), 16: SET_16, 13: SET_13}
    if num_classes not in sets:
        raise ValueError(f"prediction images are defined for 19, 16 and 13 classes, not {num_classes}")
    return list(sets[num_classes])


def id_table(num_classes):
    """uint8 [C]: class -> trainId -> Cityscapes labelId (the test server's encoding)."""
    return np.array([TRAINID_TO_ID[t] for t in trainids_of(num_classes)], np.uint8)


def palette_table(num_classes):
    """uint8 [C, 3]: class -> the RGB colour of its trainId."""
    return np.array([label_colours[t] for t in trainids_of(num_classes)], np.uint8)


def shade_table(num_classes):
    """uint8 [4, C, 3]: int(ratio * x) of every colour channel - Python's own rounding, as the reference's."""
    pal = palette_table(num_classes).tolist()
    return np.array([[[int(r * x) for x in rgb] for rgb in pal] for r in RATIOS], np.uint8)
