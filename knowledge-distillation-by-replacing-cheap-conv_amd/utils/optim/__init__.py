"""Optimizers resolvable by name from configs (`config.init_obj('optimizer', utils.optim, params)`): every torch.optim
class plus the reference's RAdam, PlainRAdam and AdamW (the reference's utils/optim/__init__.py star-imports torch.optim, then
its radam.py, the same way: `AdamW` is the reference's class here as there; torch's stays reachable as torch.optim.AdamW).  `SGD`
and `Adam` are torch's classes with the step on this package's kernel (sgd_adam.py)."""
import importlib

from torch.optim import *  # noqa: F401,F403

from .radam import AdamW, PlainRAdam, RAdam  # noqa: F401
from .sgd_adam import SGD, Adam  # noqa: F401

# torch.optim's star import also binds the name `lr_scheduler`; rebind it to this package's module
lr_scheduler = importlib.import_module(".lr_scheduler", __name__)
