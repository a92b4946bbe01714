"""Test-time augmentation: the network classifies the symmetric views of an image and the probabilities are averaged
(`HipNet.probabilities_tta`; kernels in csrc/tta.hip).  Not in the reference, which classifies every ROI once.

A view code is in 0..7, the dihedral group of the square: bit value 4 transposes H and W and is applied first, bit
value 2 then reverses the rows, bit value 1 the columns.  So 0 is the identity, 1 and 2 are the two flips, 3 the half
turn, 4 the transpose, 5 and 6 the quarter turns, 7 the anti-transpose.  The views are taken of the image the network
sees - behind `Resize`, like the training flips and rotations - so the border is part of the image.
"""

MODES = {"none": (0,), "flip": (0, 1, 2, 3), "dihedral": (0, 1, 2, 3, 4, 5, 6, 7)}


def views_of(mode):
    """The view codes of a mode name (`--tta`, `[train] test_tta`)."""
    try:
        return MODES[mode]
    except (KeyError, TypeError):
        raise ValueError(f"unknown test-time augmentation {mode!r}: one of {', '.join(MODES)}") from None


def check_shape(views, img_shape):
    """A transposing view maps an H x W image onto a W x H one: the network's input must be square for it.
    img_shape: (C, H, W), as `[image] shape` gives it."""
    h, w = int(img_shape[-2]), int(img_shape[-1])
    if h != w and any(int(v) & 4 for v in views):
        raise ValueError(f"test-time augmentation with transposed views needs a square [image] shape, got {h} x {w} "
                         f"(use `flip`)")
