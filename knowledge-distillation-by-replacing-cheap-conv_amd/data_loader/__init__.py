from .data_loaders import Cifar10Dataloader, Cifar100Dataloader  # noqa: F401
