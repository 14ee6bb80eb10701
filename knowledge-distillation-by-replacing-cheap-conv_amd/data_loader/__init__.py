from .data_loaders import Cifar10Dataloader, Cifar100Dataloader, CityscapesDataloader, CityscapesUniformDataloader  # noqa: F401
from . import joint_transforms  # noqa: F401
from . import transforms as extended_transforms
from . import transforms as standard_transforms        # the ToTensor / Normalize / Compose stand-ins live beside the extended ones


def _create_transform(config):
    """The reference's four-tuple (data_loader/__init__.py:7-51): (train joint transform, train image transform, mask transform,
    validation image transform), as parameter holders that CityscapesDataloader reads as a specification."""
    mean_std = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    jp = config['transforms']['joint_transforms']
    train_joint_transform = joint_transforms.Compose([
        joint_transforms.RandomSizeAndCrop(jp['crop_size'], False, pre_size=None, scale_min=jp['scale_min'], scale_max=jp['scale_max'],
                                           ignore_index=jp['ignore_label']),
        joint_transforms.Resize(jp['crop_size']),
        joint_transforms.RandomHorizontallyFlip()])
    ep = config['transforms']['extended_transforms']
    train_input_transform = []
    if ep['color_aug'] > 0:
        train_input_transform += [extended_transforms.ColorJitter(brightness=ep['color_aug'], contrast=ep['color_aug'],
                                                                  saturation=ep['color_aug'], hue=ep['color_aug'])]
    if ep['blur'] == 'bilateral':
        train_input_transform += [extended_transforms.RandomBilateralBlur()]
    elif ep['blur'] == 'gaussian':
        train_input_transform += [extended_transforms.RandomGaussianBlur()]
    train_input_transform += [standard_transforms.ToTensor(), standard_transforms.Normalize(*mean_std)]
    train_input_transform = standard_transforms.Compose(train_input_transform)
    val_input_transform = standard_transforms.Compose([standard_transforms.ToTensor(), standard_transforms.Normalize(*mean_std)])
    target_transform = extended_transforms.MaskToTensor()
    return train_joint_transform, train_input_transform, target_transform, val_input_transform
