"""Parameter holders with the names of the reference's data_loader/joint_transforms.py that `_create_transform` uses.  Nothing here
touches an image: CityscapesDataloader reads the objects as a specification of its fixed chain (see data_loaders.py) and the kernels
of csrc/seg_data_ops.hip do the work."""


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __repr__(self):
        return f"Compose({self.transforms!r})"


class RandomSizeAndCrop:
    """Resize by s ~ U(scale_min, scale_max) (image bicubic, mask nearest), pad where the result is smaller than the crop, then a
    uniformly placed size x size crop (reference :346-373 with RandomCrop :75-123)."""

    def __init__(self, size, crop_nopad, scale_min=0.5, scale_max=2.0, ignore_index=0, pre_size=None):
        self.size, self.crop_nopad, self.scale_min, self.scale_max = size, crop_nopad, scale_min, scale_max
        self.ignore_index, self.pre_size = ignore_index, pre_size

    def __repr__(self):
        return (f"RandomSizeAndCrop({self.size}, {self.crop_nopad}, scale_min={self.scale_min}, scale_max={self.scale_max}, "
                f"ignore_index={self.ignore_index}, pre_size={self.pre_size})")


class Resize:
    """Resize to size x size.  Behind RandomSizeAndCrop(size) the image always has that size already, so it never fires."""

    def __init__(self, size):
        self.size = (size, size)

    def __repr__(self):
        return f"Resize({self.size[0]})"


class RandomHorizontallyFlip:
    """Flip image and mask with probability 0.5."""

    def __repr__(self):
        return "RandomHorizontallyFlip()"
