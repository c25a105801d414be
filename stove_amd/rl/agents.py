"""Proximal policy optimisation on a collected batch (counterpart of the reference's model/rl/agents.py): the same arithmetic in torch
autograd with torch.optim.Adam -- ppo_epoch passes over num_mini_batch slices of a fresh torch.randperm each.  With fused=True the
same update is one launch on the device (ops.ppo_update, csrc/ppo_update.hip): the permutations are drawn exactly where the torch path
draws them, so a torch seed selects the same mini-batches on both paths.  With fused_images=True the update of the image policy
runs on the device as well (ops.ppo_update_images, csrc/ppo_image_update.hip), on a dense observation tensor (`update`) or straight on
the frames the collection wrote (`update_windows`)."""
import torch
import torch.nn as nn
import torch.optim as optim


class Agent:
    def __init__(self, actor_critic):
        pass

    def update(self):
        raise NotImplementedError


class PPOAgent(Agent):
    def __init__(self, actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr=None, eps=None,
                 max_grad_norm=None, use_clipped_value_loss=True, fused=None, fused_images=None):
        super().__init__(actor_critic)
        self.actor_critic = actor_critic
        self.clip_param = clip_param
        self.ppo_epoch = ppo_epoch
        self.num_mini_batch = num_mini_batch
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.optimizer = optim.Adam(actor_critic.parameters(), lr=lr, eps=eps)
        self.fused = bool(fused)
        if self.fused:
            shape = getattr(actor_critic, 'kernel_shape', lambda: None)()
            if shape is None:
                raise ValueError('PPOAgent: fused=True needs a policy stove_ppo_update serves: Policy(base="control") on 1 .. 6 objects with '
                                 'a head of width 1 .. 128 and nine actions (the image policy takes fused_images=True)')
        self.fused_images = bool(fused_images)
        if self.fused_images:
            if self.fused:
                raise ValueError('PPOAgent: fused=True and fused_images=True name two different policies')
            if getattr(actor_critic, 'image_kernel_shape', lambda: None)() is None:
                raise ValueError('PPOAgent: fused_images=True needs a policy stove_ppo_update_images serves: Policy((32, 32, 3 F), 9) '
                                 'without use_grid, F in 1 .. 4, with a head of width 1 .. 512 and nine actions')
        if self.fused or self.fused_images:
            self.lr, self.eps = lr, eps
            self._moments = None          # (m, v, step) as flat device tensors, made at the first update where the policy then lives

    def update(self, obs, actions, returns, values, action_log_probs, adv_targ):
        """every argument flattened to (b * n, ...) -> the value loss, action loss and entropy averaged over the optimiser steps.
        (The advantages handed in are used as they are: the normalised ones the reference computes first are never read there either.)"""
        if self.fused:
            return self._update_fused(obs, actions, returns, values, action_log_probs, adv_targ)
        if self.fused_images:
            return self._update_fused_images('update', obs, None, actions, returns, values, action_log_probs, adv_targ)
        value_loss_epoch = action_loss_epoch = dist_entropy_epoch = 0.
        n = obs.size(0)
        mb = int(n / self.num_mini_batch)
        for _ in range(self.ppo_epoch):
            perm = torch.randperm(n).to(obs.device)
            _obs, _actions, _returns = obs[perm], actions[perm], returns[perm]
            _values, _logp, _adv = values[perm], action_log_probs[perm], adv_targ[perm]
            for i in range(self.num_mini_batch):
                rows = slice(i * mb, (i + 1) * mb)
                new_values, new_logp, dist_entropy = self.actor_critic.evaluate_actions(_obs[rows], _actions[rows])
                ratio = torch.exp(new_logp - _logp[rows])
                surr1 = ratio * _adv[rows]
                surr2 = torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param) * _adv[rows]
                action_loss = -torch.min(surr1, surr2).mean()
                clipped = _values[rows] + (new_values - _values[rows]).clamp(-self.clip_param, self.clip_param)
                value_losses = (new_values - _returns[rows]).pow(2)
                value_losses_clipped = (clipped - _returns[rows]).pow(2)
                value_loss = 0.5 * torch.max(value_losses, value_losses_clipped).mean()
                self.optimizer.zero_grad()
                (value_loss * self.value_loss_coef + action_loss - dist_entropy * self.entropy_coef).backward()
                nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
                self.optimizer.step()
                value_loss_epoch += value_loss.item()
                action_loss_epoch += action_loss.item()
                dist_entropy_epoch += dist_entropy.item()
        steps = self.ppo_epoch * self.num_mini_batch
        return value_loss_epoch / steps, action_loss_epoch / steps, dist_entropy_epoch / steps

    def _update_fused(self, obs, actions, returns, values, action_log_probs, adv_targ):
        """the same update in one launch.  (use_clipped_value_loss is not read here either: the loop above always clips the value loss,
        as the reference does, and the two paths compute the same thing; stove_ppo_update itself takes the switch.)"""
        from .. import ops
        N, H, deep = self.actor_critic.kernel_shape()
        for name, ten in (('obs', obs), ('actions', actions), ('returns', returns), ('values', values), ('action_log_probs', action_log_probs),
                          ('adv_targ', adv_targ)):
            if not isinstance(ten, torch.Tensor) or not ten.is_cuda:
                raise RuntimeError('PPOAgent.update: fused=True needs %s as a tensor on the GPU (fused=None updates on the host)' % name)
        n = obs.size(0)
        if obs.dim() != 2 or obs.size(1) != 4 * N or any(t.numel() != n for t in (actions, returns, values, action_log_probs, adv_targ)):
            raise ValueError('PPOAgent.update: fused=True takes obs (n, %d) and n actions, returns, values, log-probabilities and advantages' % (4 * N))
        if any(t.is_floating_point() and t.dtype != torch.float32 for t in (obs, returns, values, action_log_probs, adv_targ)):
            raise ValueError('PPOAgent.update: fused=True takes float32 tensors')
        if n < self.num_mini_batch:
            raise ValueError('PPOAgent.update: %d rows do not make %d mini-batches' % (n, self.num_mini_batch))
        dev = obs.device
        perm = torch.stack([torch.randperm(n) for _ in range(self.ppo_epoch)]) if self.ppo_epoch else torch.zeros((0, n), dtype=torch.int64)
        image = self.actor_critic.flat_params()
        if image.device != dev:
            raise ValueError('PPOAgent.update: the policy lives on %s, the batch on %s' % (image.device, dev))
        if self._moments is None or self._moments[0].device != dev:
            self._moments = (torch.zeros_like(image), torch.zeros_like(image), torch.zeros(1, dtype=torch.int32, device=dev))
        m, v, step = self._moments
        flat = lambda t: t.detach().reshape(n).contiguous()
        out = ops.ppo_update(image, m, v, step, obs.detach().contiguous(), flat(actions).to(torch.int32), flat(returns), flat(values),
                             flat(action_log_probs), flat(adv_targ), perm.to(device=dev, dtype=torch.int32), self.num_mini_batch, H, deep,
                             self.clip_param, self.value_loss_coef, self.entropy_coef, self.lr, self.eps, self.max_grad_norm, True)
        self.actor_critic.load_flat_params(image)
        steps = self.ppo_epoch * self.num_mini_batch
        if steps == 0:
            return 0., 0., 0.
        host = torch.cat([out['losses'].sum(0).double(), out['status'].double()]).cpu()          # (the one synchronisation)
        if int(host[3]) != 0:
            raise RuntimeError('PPOAgent.update: optimiser step %d of %d stopped the fused update with status %d (3: a loss or the '
                               'gradient norm was not finite; 2: an index out of range); the policy stands as the step before left it'
                               % (int(host[4]), steps, int(host[3])))
        return float(host[0]) / steps, float(host[1]) / steps, float(host[2]) / steps

    def update_windows(self, frames, S, actions, returns, values, action_log_probs, adv_targ):
        """the update of a fused_images agent straight on the collection's frames (B, F + S, 3, 32, 32): row b S + s of the n = B S rows
        is the window frames[b, s:s + F], which is never copied -> as update"""
        if not self.fused_images:
            raise ValueError('PPOAgent.update_windows: the agent was not built with fused_images=True')
        return self._update_fused_images('update_windows', frames, int(S), actions, returns, values, action_log_probs, adv_targ)

    def _update_fused_images(self, who, obs, S, actions, returns, values, action_log_probs, adv_targ):
        """S None: obs dense (n, 3F, 32, 32); else obs the frames (B, F + S, 3, 32, 32)"""
        from .. import ops
        F, H, deep = self.actor_critic.image_kernel_shape()
        for name, ten in (('obs' if S is None else 'frames', obs), ('actions', actions), ('returns', returns), ('values', values),
                          ('action_log_probs', action_log_probs), ('adv_targ', adv_targ)):
            if not isinstance(ten, torch.Tensor) or not ten.is_cuda:
                raise RuntimeError('PPOAgent.%s: fused_images=True needs %s as a tensor on the GPU (fused_images=None updates on the host)'
                                   % (who, name))
        if S is None:
            if obs.dim() != 4 or tuple(obs.shape[1:]) != (3 * F, 32, 32):
                raise ValueError('PPOAgent.update: fused_images=True takes obs (n, %d, 32, 32)' % (3 * F))
            n = obs.size(0)
        else:
            if S < 1 or obs.dim() != 5 or tuple(obs.shape[1:]) != (F + S, 3, 32, 32):
                raise ValueError('PPOAgent.update_windows: frames of S = %d steps must be (B, %d, 3, 32, 32)' % (S, F + S))
            n = obs.size(0) * S
        if any(t.numel() != n for t in (actions, returns, values, action_log_probs, adv_targ)):
            raise ValueError('PPOAgent.%s: %d rows need as many actions, returns, values, log-probabilities and advantages' % (who, n))
        if any(t.is_floating_point() and t.dtype != torch.float32 for t in (obs, returns, values, action_log_probs, adv_targ)):
            raise ValueError('PPOAgent.%s: fused_images=True takes float32 tensors' % who)
        if n < self.num_mini_batch:
            raise ValueError('PPOAgent.%s: %d rows do not make %d mini-batches' % (who, n, self.num_mini_batch))
        dev = obs.device
        perm = torch.stack([torch.randperm(n) for _ in range(self.ppo_epoch)]) if self.ppo_epoch else torch.zeros((0, n), dtype=torch.int64)
        image = self.actor_critic.flat_image_params()
        if image.device != dev:
            raise ValueError('PPOAgent.%s: the policy lives on %s, the batch on %s' % (who, image.device, dev))
        if self._moments is None or self._moments[0].device != dev:
            self._moments = (torch.zeros_like(image), torch.zeros_like(image), torch.zeros(1, dtype=torch.int32, device=dev))
        m, v, step = self._moments
        flat = lambda t: t.detach().reshape(n).contiguous()
        out = ops.ppo_update_images(image, m, v, step, obs.detach().contiguous(), flat(actions).to(torch.int32), flat(returns), flat(values),
                                    flat(action_log_probs), flat(adv_targ), perm.to(device=dev, dtype=torch.int32), self.num_mini_batch, F, H,
                                    deep, self.clip_param, self.value_loss_coef, self.entropy_coef, self.lr, self.eps, self.max_grad_norm, True,
                                    steps_per_env=S)
        self.actor_critic.load_flat_image_params(image)
        steps = self.ppo_epoch * self.num_mini_batch
        if steps == 0:
            return 0., 0., 0.
        host = torch.cat([out['losses'].sum(0).double(), out['status'].double()]).cpu()          # (the one synchronisation)
        if int(host[3]) != 0:
            raise RuntimeError('PPOAgent.update: optimiser step %d of %d stopped the fused update with status %d (3: a loss or the '
                               'gradient norm was not finite; 2: an index out of range); the policy stands as the step before left it'
                               % (int(host[4]), steps, int(host[3])))
        return float(host[0]) / steps, float(host[1]) / steps, float(host[2]) / steps
