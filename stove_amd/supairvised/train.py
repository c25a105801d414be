"""Trainer of the state-supervised baseline (reference model/supairvised/train.py: SupTrainer :14-495).

Same public surface -- `SupTrainer(config, stove, train_dataset, test_dataset)` with `compute_loss`, `error_and_log`,
`prediction_error`, `its`, `train`, `test`, `long_rollout` -- the same six-column log and the same order of test / save / long rollout.
Optimiser, arena, loaders and checkpoints are AbstractTrainer's.  Not built: SuPAIR-state supervision (`load_encoder`, the reference's
Supervisor and match_positions) and the gif animation of long rollouts (no plotting in this package).
"""
import os
import time

import numpy as np
import torch
from torch import nn

from .. import ops
from ..optim import FlatAdam
from ..utils.utils import ExperimentLogger
from ..video_prediction.train import AbstractTrainer
from .supstove import NO_SUPERVISOR


class SupTrainer(AbstractTrainer):
    def __init__(self, config, stove, train_dataset, test_dataset):
        if config.load_encoder is not None:
            raise NotImplementedError(NO_SUPERVISOR)
        super().__init__(config, stove, train_dataset, test_dataset)
        # types are: vin_true (model against true states); frame is: total, pred, recon
        attributes = ['step', 'time', 'error', 'type', 'frame', 'test']
        log_str = '{:d},' + 2 * '{:.5f},' + 2 * '{},' + '{}\n'
        self.logger = ExperimentLogger(config, attributes, log_str)

    def compute_loss(self, present_labels, future_labels, recons, preds):
        """-> (total, pred_loss, recon_loss): discounted MSE of the predicted states and of their frame-to-frame differences, plus
        the reconstruction term (zero here: the model returns the given states as its reconstruction)."""
        df = self.c.discount_factor
        end = 2 if self.c.debug_disable_v_error else 4
        with_delta = not self.c.debug_disable_v_diff_error
        loss = nn.MSELoss()
        recon_loss = loss(recons[..., :end], present_labels[..., :end])
        if preds.is_cuda and preds.dtype == torch.float32:
            total, pred_loss, _ = ops.sup_loss(preds, future_labels, df, end, with_delta)
            return total + recon_loss, pred_loss, recon_loss
        delta_labels = future_labels[:, 1:] - future_labels[:, :-1]
        delta_preds = preds[:, 1:] - preds[:, :-1]
        num_rollout = preds.shape[1]
        pred_loss, delta_pred_loss = 0.0, 0.0
        for t in range(num_rollout):
            pred_loss = pred_loss + df ** (t + 1) * loss(preds[:, t, :, :end], future_labels[:, t, :, :end])
            if with_delta and t < num_rollout - 1:
                delta_pred_loss = delta_pred_loss + df ** (t + 1) * 6 * loss(delta_preds[:, t, :, :end], delta_labels[:, t, :, :end])
        return pred_loss + recon_loss + delta_pred_loss, pred_loss, recon_loss

    def prediction_error(self, predicted, real, suffix=''):
        """Append the mean and the standard deviation over the sequences of the per-frame position error to error{suffix}.csv and
        std_error{suffix}.csv."""
        if suffix != '' and suffix[0] != '_':
            suffix = '_' + suffix
        tmp = torch.sqrt(((predicted[..., :2] - real[..., :2]) ** 2).sum(-1)).mean(-1)
        for name, data in (('error', tmp.mean(0)), ('std_error', tmp.std(0))):
            with open(os.path.join(self.logger.exp_dir, '{}{}.csv'.format(name, suffix)), 'a') as f:
                f.write(','.join(['{:.6f}'.format(i) for i in data]) + '\n')

    @staticmethod
    def its(states):
        """Inverse of the dataset's rescaling, to the [-1, 1] frame: positions were [0, 10] / 5, velocities * 2."""
        pos = states[..., :2] * 5
        vel = states[..., 2:4] / 2
        return torch.cat([pos / 10 * 2 - 1, vel / 10 * 2], -1)

    def _labels(self, data):
        return self.init_t(data['present_labels']), self.init_t(data['future_labels'])

    def train_step(self, data, latent=None):
        """One optimisation step on a batch dict -> (total, pred_loss, recon_loss)."""
        present, future = self._labels(data)
        self.bucket.zero()
        pred, recon = self.stove.dyn(present, num_rollout=self.c.num_rollout, debug_rollout=self.c.debug_rollout_training, latent=latent)
        total, pred_loss, recon_loss = self.compute_loss(present, future, recon, pred)
        total.backward()
        self.bucket.all_reduce()
        if isinstance(self.optimizer, FlatAdam):
            self.optimizer.step(max_norm=None)
        else:
            self.optimizer.step()
        return total.detach(), pred_loss.detach(), recon_loss.detach()

    def train(self):
        print('Supervised!')
        if self.c.action_conditioned:
            raise NotImplementedError('the supervised baseline is not action-conditioned')
        step_counter = self.step_start
        start = time.time()
        self.test(step_counter, start)
        epoch = self.epoch_start
        for epoch in range(self.epoch_start, self.c.num_epochs):
            for data in self.dataloader:
                if self.c.debug_anneal_lr:
                    self.adjust_learning_rate(self.optimizer, self.c.debug_anneal_lr, step_counter)
                now = time.time() - start
                step_counter += 1
                total, pred_loss, recon_loss = self.train_step(data)
                if step_counter % self.c.print_every == 0:
                    self.error_and_log({'step': step_counter, 'time': now}, total.item(), pred_loss.item(), recon_loss.item(), 'vin_true')
                if self.c.debug_test_mode:
                    break
                if step_counter % self.c.save_every == 0:
                    self.save(epoch, step_counter)
                if step_counter % self.c.long_rollout_every == 0:
                    self.long_rollout(idx=[0, 1], step_counter=step_counter)
            if self.c.debug_test_mode:
                break
            self.test(step_counter, start)
            print('epoch ', epoch, ' Finished')
        if not self.c.debug_test_mode:
            self.long_rollout(step_counter=step_counter)
        if not self.c.nolog:
            self.save(epoch, step_counter)
            open(os.path.join(self.logger.exp_dir, 'success'), 'w').close()
        print('Finished Training')

    def error_and_log(self, perf_dict, total_loss, pred_loss, recon_loss, log_type, test=False):
        """One log row per frame (total, pred, recon) of an error type."""
        for error, frame in zip((total_loss, pred_loss, recon_loss), ('total', 'pred', 'recon')):
            perf_dict['error'] = error
            perf_dict['type'] = log_type
            perf_dict['frame'] = frame
            perf_dict['test'] = str(test)
            self.logger.performance(perf_dict)

    @torch.no_grad()
    def test(self, step_counter, start):
        """The loss on up to nine batches of the test set."""
        self.stove.eval()
        perf_dict = {'step': step_counter, 'time': time.time() - start}
        for i, data in enumerate(self.test_dataloader):
            present, future = self._labels(data)
            pred, recon = self.stove.dyn(present, num_rollout=self.c.num_rollout, debug_rollout=self.c.debug_rollout)
            total, pred_loss, recon_loss = self.compute_loss(present, future, recon, pred)
            self.error_and_log(perf_dict, total.item(), pred_loss.item(), recon_loss.item(), 'vin_true', test=True)
            if self.c.debug_test_mode or i > 7:
                break
        self.stove.train()

    @torch.no_grad()
    def long_rollout(self, idx=None, actions=None, step_counter=None, num=500):
        """Roll every test sequence out for `num` steps from its first num_visible states; log the position error over the frames the
        test set covers and save the states.  (idx chose the sequences the reference animates; there is no animation here.)"""
        if actions is not None or self.c.action_conditioned:
            raise NotImplementedError('the supervised baseline is not action-conditioned')
        total_labels = self.test_dataset.total_data
        step, visible = self.c.frame_step, self.c.num_visible
        max_rollout = min(self.c.num_frames // step - visible, num)
        true_states = self.init_t(torch.as_tensor(total_labels[:, :visible * step:step]))
        pred, recon = self.stove.dyn(true_states, num_rollout=num, debug_rollout=self.c.debug_rollout)
        simu = torch.cat([recon, pred], 1)
        real_labels = self.init_t(torch.as_tensor(total_labels[:, :(visible + max_rollout) * step:step]))
        self.prediction_error(simu[:, :visible + max_rollout], real_labels)
        add = [''] if step_counter is None else ['', '_{:05d}'.format(step_counter)]
        for a in add:
            np.save(os.path.join(self.logger.rollout_states_dir, 'rollout_states' + a), simu.cpu().numpy())
        np.save(os.path.join(self.logger.rollout_states_dir, 'real_states'), real_labels.cpu().numpy())
