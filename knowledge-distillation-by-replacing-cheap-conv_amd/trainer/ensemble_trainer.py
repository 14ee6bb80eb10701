"""`EnsembleTrainer` (reference trainer/ensemble_trainer.py:12-205): a student distilled from the teacher AND from K frozen
students that earlier runs produced (`trainer.resume_paths`), and the evaluation of that ensemble (`trainer.test()`,
train_classification.py:63-71).  Classification students only (the module-graph path of DepthwiseStudent), as in the reference.

Kept from the reference on purpose:
  * `resume_ensemble` rebuilds each member by replaying its checkpoint's plan on THIS model, loading the checkpoint (student.* and
    teacher.* entries alike), copying the student and calling `model.reset()`, which only puts the replaced blocks back.  The student
    that is trained afterwards therefore starts from the last checkpoint's weights in every layer that was not replaced;
  * loss = kd_loss + supervised_loss, kd_loss = (sum_k WEIGHT * KD(s, member_k) + KD(s, teacher)) / (WEIGHT * K + 1);
  * `len_epoch + 1` iterations, optimizer step on (batch_idx + 1) % accumulation_steps, validation of the single student (`val_*`)
    and of the ensemble (`ensemble_*`) after the epoch.

Re-designed for the GPU: with KLDivergenceLoss and a plain CrossEntropyLoss2d the K + 1 KL terms, the cross entropy, their sum and
its gradient are one kd_kldiv_multi call (include/kdcc.h) behind one autograd Function -- the student logits are read once instead of
2K + 4 times and there is one gradient buffer instead of K + 2; `ensemble_predict` is one kd_softmax_mean call; metrics are summed on
the device (no .item() per step).  Any other pair of criteria takes the reference's loop over the criterion modules."""
import copy
from functools import reduce

import torch

from .. import ops
from ..losses import CrossEntropyLoss2d, KLDivergenceLoss
from ..models import forgiving_state_restore
from ..parallel import mean_scalar
from ..utils.optim.lr_scheduler import MyOneCycleLR, MyReduceLROnPlateau
from .classification_trainer import ClassificationTrainer

WEIGHT = 1
TEMPERATURE = 1       # ensemble_predict only; the training criterion's temperature is criterions[1].temperature


class _EnsembleCriterion(torch.autograd.Function):
    """(total, kd, sup) of kd_kldiv_multi; d total / d logits is computed with them and only scaled in backward."""

    @staticmethod
    def forward(ctx, logits, labels, temperature, ignore_index, scale, weights, *targets):
        kd, sup, total, grad = ops.kldiv_multi(logits.detach(), [t.detach() for t in targets], weights, temperature, labels,
                                               ignore_index, scale, scale, want_grad=logits.requires_grad)
        ctx.grad = grad
        ctx.mark_non_differentiable(kd, sup)
        return total, kd, sup

    @staticmethod
    def backward(ctx, g, _g_kd, _g_sup):
        grad, ctx.grad = ctx.grad, None
        rest = (None,) * 5 + (None,) * (len(ctx.needs_input_grad) - 6)
        if grad is None:
            return (None,) + rest
        if g.numel() == 1 and grad.data_ptr() % 16 == 0:
            return (ops.scale_by_device_scalar_(grad, g),) + rest
        return (grad * g.to(grad.dtype),) + rest


class EnsembleTrainer(ClassificationTrainer):
    def __init__(self, model, criterions, metric_ftns, optimizer, config, train_data_loader, valid_data_loader=None,
                 lr_scheduler=None, weight_scheduler=None, test_data_loader=None):
        if getattr(model, 'fused', False):
            raise NotImplementedError("EnsembleTrainer supports classification students only (the reference's scope): "
                                      f"{type(model.student).__name__} runs on the fused engine")
        super().__init__(model, criterions, metric_ftns, optimizer, config, train_data_loader, valid_data_loader, lr_scheduler,
                         weight_scheduler, test_data_loader)
        if 'resume_paths' not in self.config['trainer']:
            raise ValueError("Cannot find path to checkpoints, please specify them by adding 'resume_paths' in config.trainer")
        self.models = []
        self.resume_ensemble(self.config['trainer']['resume_paths'])

    def resume_ensemble(self, checkpoint_paths):
        for index, checkpoint_path in enumerate(checkpoint_paths):
            self.logger.info("Loading checkpoint: {} ...".format(checkpoint_path))
            # (`config` is a pickled ConfigParser in this package's checkpoints, a plain dict in exported ones: both index alike)
            checkpoint = torch.load(str(checkpoint_path), map_location=torch.device('cpu'), weights_only=False)
            config, epoch = checkpoint['config'], checkpoint['epoch']
            for i in range(1, epoch + 1):                 # align the network: replay the checkpoint's plan
                self.prepare_train_epoch(i, config)
            forgiving_state_restore(self.model, checkpoint['state_dict'])
            self.logger.info("Loaded state dict for model {}".format(index))
            self.models.append(copy.deepcopy(self.model.student))
            self.model.reset()                            # replaced blocks only (see the module docstring)
        self.logger.info('loaded state dict for all models')

    def prepare_models(self, epoch):
        for param in self.model.student.parameters():
            param.requires_grad = True
        for param in self.model.teacher.parameters():
            param.requires_grad = False
        for member in self.models:
            for param in member.parameters():
                param.requires_grad = False
            member.eval()
        self.model.train()
        if epoch == 1:
            self.create_new_optimizer()
            self.logger.debug(self.model.student)
        self._reducer = None                              # trainable set changed: rebuild the gradient buckets lazily

    # ------------------------------------------------------------------ criterion
    def _fused_criterion(self):
        sup, kd = self.criterions[0], self.criterions[1]
        return type(kd) is KLDivergenceLoss and type(sup) is CrossEntropyLoss2d and sup.weight is None and sup.size_average

    def _criterion(self, output_st, output_tc, outputs, target):
        """-> (loss to back-propagate, then what is logged: loss, supervised_loss, kd_loss before the division by accumulation_steps)
        (reference :80-85, :95-97)."""
        acc = self.accumulation_steps
        if self._fused_criterion() and output_st.is_cuda:
            weights = [float(WEIGHT)] * len(outputs) + [1.0]
            total, kd, sup = _EnsembleCriterion.apply(output_st, target, float(self.criterions[1].temperature),
                                                      self.criterions[0].ignore_index, 1.0 / acc, weights, *outputs, output_tc)
            return total, (total.detach() * acc if acc != 1 else total.detach()), sup, kd
        supervised_loss = self.criterions[0](output_st, target) / acc
        kd_loss = reduce(lambda a, elem: a + WEIGHT * self.criterions[1](output_st, elem), outputs, 0)
        kd_loss = kd_loss + self.criterions[1](output_st, output_tc)
        kd_loss = kd_loss / (WEIGHT * len(outputs) + 1) / acc
        loss = kd_loss + supervised_loss
        return loss, loss.detach() * acc, supervised_loss.detach() * acc, kd_loss.detach() * acc

    def _train_epoch(self, epoch):
        self.prepare_models(epoch)
        self.train_metrics.reset()
        self._clean_cache()
        self._attach_reducer()
        for batch_idx, (data, target) in enumerate(self.train_data_loader):
            data, target = data.to(self.device), target.to(self.device)
            output_st, output_tc = self.model(data)
            with torch.no_grad():
                outputs = [member(data) for member in self.models]
            loss, log_loss, log_supervised, log_kd = self._criterion(output_st, output_tc, outputs, target)
            loss.backward()
            self._reduce_unfused_grads()
            if (batch_idx + 1) % self.accumulation_steps == 0:
                self.optimizer.step()
                self.optimizer.zero_grad()
            self.writer.set_step((epoch - 1) * self.len_epoch + batch_idx)
            self.train_metrics.update('loss', log_loss)
            self.train_metrics.update('supervised_loss', log_supervised)
            self.train_metrics.update('kd_loss', log_kd)
            for met in self.metric_ftns:
                self.train_metrics.update(met.__name__, met(output_st, target))
                self.train_teacher_metrics.update(met.__name__, met(output_tc, target))
            if batch_idx % self.log_step == 0:
                self.train_metrics.flush()
            if batch_idx % self.log_step == 0 and self.rank == 0:
                first = self.metric_ftns[0].__name__ if self.metric_ftns else None
                self.logger.info('Train Epoch: {} [{}]/[{}] acc: {:.6f} teacher_acc: {:.6f} Loss: {:.6f} Supervised Loss: {:.6f} '
                                 'Knowledge Distillation loss: {:.6f}'.format(
                                     epoch, batch_idx, self.len_epoch, self.train_metrics.avg(first) if first else 0.0,
                                     self.train_teacher_metrics.avg(first) if first else 0.0, self.train_metrics.avg('loss'),
                                     self.train_metrics.avg('supervised_loss'), self.train_metrics.avg('kd_loss')))
            if batch_idx == self.len_epoch:
                break
        self.train_metrics.flush()
        log = self.train_metrics.result()
        if self.do_validation and ((epoch % self.do_validation_interval) == 0):
            self._clean_cache()
            val_log = self._valid_epoch(epoch)                 # the single student
            log.update(**{'val_' + k: v for k, v in val_log.items()})
            tc_log = self._test_epoch(epoch)                   # the ensemble
            log.update(**{'ensemble_' + k: v for k, v in tc_log.items()})
        if (self.lr_scheduler is not None) and (not isinstance(self.lr_scheduler, MyOneCycleLR)):
            if isinstance(self.lr_scheduler, MyReduceLROnPlateau):
                self.lr_scheduler.step(mean_scalar(self.train_metrics.avg('loss')))
            else:
                self.lr_scheduler.step()
        self.weight_scheduler.step()
        return log

    # ------------------------------------------------------------------ evaluation
    def ensemble_predict(self, data, weight=WEIGHT):
        """(B,3,H,W) -> probabilities (B,C): (softmax(teacher) + weight * sum_k softmax(member_k)) / (1 + K * weight), temperature
        TEMPERATURE (reference :145-164)."""
        with torch.no_grad():
            logits = [self.model.teacher(data)] + [member(data) for member in self.models]
            return ops.softmax_mean(logits, [1.0] + [float(weight)] * len(self.models), float(TEMPERATURE))

    def _valid_epoch(self, epoch):
        self.model.eval()
        self.model.save_hidden = False
        self.valid_metrics.reset()
        with torch.no_grad():
            for batch_idx, (data, target) in enumerate(self.valid_data_loader):
                data, target = data.to(self.device), target.to(self.device)
                output, _ = self.model(data)
                self.writer.set_step((epoch - 1) * len(self.valid_data_loader) + batch_idx, 'valid')
                for met in self.metric_ftns:
                    self.valid_metrics.update(met.__name__, met(output, target))
        self.valid_metrics.flush()
        return self.valid_metrics.result()

    def _test_epoch(self, epoch):
        for member in self.models:
            member.eval()
        self.model.teacher.eval()
        self.test_metrics.reset()
        with torch.no_grad():
            for batch_idx, (data, target) in enumerate(self.valid_data_loader):
                data, target = data.to(self.device), target.to(self.device)
                output = self.ensemble_predict(data)
                for met in self.metric_ftns:
                    self.test_metrics.update(met.__name__, met(output, target), data.shape[0])
        self.test_metrics.flush()
        return self.test_metrics.result()
