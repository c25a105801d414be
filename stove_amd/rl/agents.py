"""Proximal policy optimisation on a collected batch (counterpart of the reference's model/rl/agents.py): the same arithmetic in torch
autograd with torch.optim.Adam -- ppo_epoch passes over num_mini_batch slices of a fresh torch.randperm each."""
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
                 max_grad_norm=None, use_clipped_value_loss=True):
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

    def update(self, obs, actions, returns, values, action_log_probs, adv_targ):
        """every argument flattened to (b * n, ...) -> the value loss, action loss and entropy averaged over the optimiser steps.
        (The advantages handed in are used as they are: the normalised ones the reference computes first are never read there either.)"""
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
