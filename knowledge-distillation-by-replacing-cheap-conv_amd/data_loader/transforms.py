"""Parameter holders with the names of the reference's data_loader/transforms.py (its `extended_transforms`) and of the two
torchvision transforms `_create_transform` uses.  Read as a specification by CityscapesDataloader; nothing here touches an image."""


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __repr__(self):
        return f"Compose({self.transforms!r})"


class ColorJitter:
    """Brightness, contrast and saturation factors from U(max(0, 1 - a), 1 + a), hue from U(-a, a), applied in a random order."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness, self.contrast, self.saturation, self.hue = brightness, contrast, saturation, hue

    def __repr__(self):
        return f"ColorJitter({self.brightness}, {self.contrast}, {self.saturation}, {self.hue})"


class RandomGaussianBlur:
    """Gaussian blur with sigma = 0.15 + U * 1.15."""

    def __repr__(self):
        return "RandomGaussianBlur()"


class RandomBilateralBlur:
    """Named so that a config asking for it is refused by name: the loader does not implement it."""

    def __repr__(self):
        return "RandomBilateralBlur()"


class MaskToTensor:
    """The mask as an int64 tensor."""

    def __repr__(self):
        return "MaskToTensor()"


class ToTensor:
    def __repr__(self):
        return "ToTensor()"


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = tuple(mean), tuple(std)

    def __repr__(self):
        return f"Normalize({self.mean}, {self.std})"
