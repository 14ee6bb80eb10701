"""`AnalysisTrainer`: which layers are compressible (trainer/analysis_trainer.py:6-138 of the reference).  For every entry of
config['layer_compressible'] and every learning rate: the layer is replaced by the probe block (AnalysisStudent.replace), its 1x1
is trained on the hint loss alone for `epochs - 1` epochs while the student's and the teacher's mIoU and their gap are logged, and
the student is reset.  Reference behaviour kept on purpose: `range(1, self.epochs)` (:37), scheduler reset and a new optimizer per
learning rate with that rate written into every param group (:28-32), `model.reset()` after each learning rate (:39).

Losses stay device scalars and the confusion matrices stay on the device, as in LayerwiseTrainer._train_epoch.  With
`trainer.fused_metrics: true` (opt-in) a step's logged numbers come from one HIP pass over the two half-resolution LazyLogits
(ops.logit_metrics_up: both cross entropies, the logit MSE, both confusion matrices) and neither full-resolution tensor is ever
materialised; by default the criteria and two kd_confusion passes are composed, as the reference composes them (:55-81)."""
from ..lazy import LazyLogits
from ..losses import CrossEntropyLoss2d, MSELoss
from ..parallel import mean_scalar
from ..utils.optim.lr_scheduler import MyOneCycleLR, MyReduceLROnPlateau
from .layerwise_trainer import LayerwiseTrainer


class AnalysisTrainer(LayerwiseTrainer):
    def __init__(self, model, criterions, metric_ftns, optimizer, config, train_data_loader, valid_data_loader=None,
                 lr_scheduler=None, weight_scheduler=None):
        super().__init__(model, criterions, metric_ftns, optimizer, config, train_data_loader, valid_data_loader, lr_scheduler,
                         weight_scheduler)
        # trainer.fused_metrics: true takes a step's logged numbers from one pass over the half-resolution logits
        # (ops.logit_metrics_up).  Opt-in: it has not been timed against the composition it replaces (tools/bench_analysis.py)
        self.fused_metrics = bool(self.config['trainer'].get('fused_metrics', False))
        self.fused_metric_steps = 0

    def train(self):
        for layer in self.config['layer_compressible']:
            layer_name, lrs, args = layer['layer_name'], layer['lrs'], layer['args']
            for lr in lrs:
                self.logger.info(f'Replacing layer: {layer_name} learning rate: {lr:.6f}')
                self.model.replace([layer_name], **args)
                self.model.register_hint_layers([layer_name])
                self.reset_scheduler()
                self.create_new_optimizer()
                for param_group in self.optimizer.param_groups:
                    param_group['lr'] = lr
                self._reducer = None
                self.logger.info(self.model.dump_trainable_params())
                self.logger.info(self.model.dump_student_teacher_blocks_info())
                for epoch in range(1, self.epochs):
                    self._train_epoch(epoch, lr=lr, layer_name=layer_name)
                self.model.reset()

    def _fused_ok(self, output_st, output_tc):
        c0, c1 = self.criterions[0], self.criterions[1]
        return (self.fused_metrics and self.track_miou and
                isinstance(output_st, LazyLogits) and isinstance(output_tc, LazyLogits) and output_st.pending and output_tc.pending and
                output_st.size_hw == output_tc.size_hw and output_st.align_corners == output_tc.align_corners and
                output_st.low.shape == output_tc.low.shape and
                output_st.shape[1] == self.train_iou_metrics.num_classes and
                type(c0) is CrossEntropyLoss2d and c0.weight is None and c0.size_average and
                type(c1) is MSELoss and c1.reduction == 'mean')

    def _logged_metrics(self, output_st, output_tc, target):
        """(supervised, kd, teacher) losses of the step, both mIoU trackers updated: one pass over the half-resolution logits
        where that applies, the criteria and two confusion passes otherwise (and where the kernel refuses the shape)."""
        if self._fused_ok(output_st, output_tc):
            from .. import ops
            try:
                out, conf_s, conf_t = ops.logit_metrics_up(output_st.low, output_tc.low, target, output_st.size_hw,
                                                           self.criterions[0].ignore_index, output_st.align_corners)
                self.train_iou_metrics.add_confusion(conf_s)
                self.train_teacher_iou_metrics.add_confusion(conf_t)
                self.fused_metric_steps += 1
                return out[0], out[2] * float(self.criterions[1].num_classes), out[1]
            except ops.MetricsUnsupported:
                pass
        supervised = self.criterions[0](output_st, target)
        kd = self.criterions[1](output_st, output_tc)
        teacher = self.criterions[0](output_tc, target)
        if self.track_miou:
            self.train_iou_metrics.update(output_st, target)
            self.train_teacher_iou_metrics.update(output_tc, target)
        return supervised, kd, teacher

    def _train_epoch(self, epoch, **kwargs):
        self.model.save_hidden = True
        self.train_metrics.reset()
        self.train_iou_metrics.reset()
        self.train_teacher_iou_metrics.reset()
        self._clean_cache()
        self._attach_reducer()
        tag = str(kwargs.get('layer_name', '')).replace('.', '_')
        lr_key = str(kwargs.get('lr'))

        for batch_idx, (data, target, _) in enumerate(self._device_batches(self.train_data_loader, False)):
            output_st, output_tc = self.model(data)

            acc = self.accumulation_steps
            supervised_loss, kd_loss, teacher_loss = self._logged_metrics(output_st, output_tc, target)
            supervised_loss, kd_loss = supervised_loss / acc, kd_loss / acc
            hint_loss = self._hint_loss() / acc

            loss = hint_loss                                        # only use hint loss (reference :64-66)
            loss.backward()
            self._reduce_unfused_grads()
            if batch_idx % self.accumulation_steps == 0:
                self.optimizer.step()
                self.optimizer.zero_grad()
            self.writer.set_step((epoch - 1) * self.len_epoch + batch_idx)

            self.train_metrics.update('loss', loss.detach() * acc)
            self.train_metrics.update('supervised_loss', supervised_loss.detach() * acc)
            self.train_metrics.update('kd_loss', kd_loss.detach() * acc)
            self.train_metrics.update('hint_loss', hint_loss.detach() * acc)
            self.train_metrics.update('teacher_loss', teacher_loss.detach())
            for met in self.metric_ftns:
                self.train_metrics.update(met.__name__, met(output_st, target))

            if batch_idx % self.log_step == 0:
                self.train_metrics.flush()   # buffered device scalars -> TensorBoard, one host sync per log point
                st_iou, tc_iou = self.train_iou_metrics.get_iou(), self.train_teacher_iou_metrics.get_iou()
                self.writer.add_scalars("mIoU/" + tag, {lr_key: st_iou}, batch_idx)
                self.writer.add_scalars("loss/" + tag, {lr_key: float(loss.detach())}, batch_idx)
                self.writer.add_scalars("student_teacher_iou_gap/" + tag, {lr_key: tc_iou - st_iou}, batch_idx)
                if self.rank == 0:
                    self.logger.info(
                        'Train Epoch: {} [{}]/[{}] Loss: {:.6f} mIoU: {:.6f} Teacher mIoU: {:.6f} Supervised Loss: {:.6f} '
                        'Knowledge Distillation loss: {:.6f} Hint Loss: {:.6f} Teacher Loss: {:.6f}'.format(
                            epoch, batch_idx, self.len_epoch, self.train_metrics.avg('loss'), st_iou, tc_iou,
                            self.train_metrics.avg('supervised_loss'), self.train_metrics.avg('kd_loss'),
                            self.train_metrics.avg('hint_loss'), self.train_metrics.avg('teacher_loss')))
            if batch_idx == self.len_epoch:
                break

        self.train_metrics.flush()
        log = self.train_metrics.result()
        log.update({'train_teacher_mIoU': self.train_teacher_iou_metrics.get_iou()})
        log.update({'train_student_mIoU': self.train_iou_metrics.get_iou()})
        if self.do_validation and ((epoch % self.config["trainer"]["do_validation_interval"]) == 0):
            val_log = self._valid_epoch(epoch)
            log.update(**{'val_' + k: v for k, v in val_log.items()})
            log.update(**{'val_mIoU': self.valid_iou_metrics.get_iou()})
            self.val_iou_tracker.update(self.valid_iou_metrics.get_iou())
        self._teacher_student_iou_gap = self.train_teacher_iou_metrics.get_iou() - self.train_iou_metrics.get_iou()

        if (self.lr_scheduler is not None) and (not isinstance(self.lr_scheduler, MyOneCycleLR)):
            if isinstance(self.lr_scheduler, MyReduceLROnPlateau):
                self.lr_scheduler.step(mean_scalar(self.train_metrics.avg('loss')))
            else:
                self.lr_scheduler.step()
        self.weight_scheduler.step()
        return log
