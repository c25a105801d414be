"""Collect a batch of trajectories on states and update the policy (counterpart of the reference's model/rl/runners.py, the
`--use-states` path).  The reference walks its batch_size environments one after the other, num_steps each, with a one-row
`Policy.act`, a `.cpu()` and a numpy step per step.  Here the batch_size start states are drawn first, exactly as the reference draws
them (`reset()` plus one step with action 0 on the one environment object, in order), and then stepped together:

  on a device, one ops.ppo_collect launch (stove_ppo_collect) when the policy is one the kernel serves, else -- or with fused=False --
  composed: per step one batched `policy.act` and one `BatchedAvoidance.step(render=False)`, nothing synchronised;
  on the host, `collect.PolicyForest`, the numpy specification of that kernel.

The arm on images (`run_batch`, the reference's default) has the same shape: the start states are drawn with `env.reset()`, the four
steps with action 0 that fill the frame buffer and the S steps on rendered frames are one ops.ppo_collect_images launch
(stove_ppo_collect_images) on a device when the policy is one that kernel serves, else a composed loop of batched `policy.act` and
`BatchedAvoidance.step(render=True)` calls, on the device or on the host; `collect.ImageForest` is that kernel's numpy specification.

All three draw action s of environment b from the same uniform u[b][s] (collect.py says why the reference's stream is not
reproduced), so they agree action for action wherever no draw sits within rounding of a boundary.  Logging goes to an optional
`writer` with an `add_scalar(key, value, step)` method (a tensorboardX SummaryWriter fits); none is required."""
import numpy as np
import torch

from ..envs.batched import BatchedAvoidance
from . import collect as _collect


class BatchStorage:
    def __init__(self, batch_size, num_steps, obs_shape, device):
        self.obs = torch.zeros((batch_size, num_steps + 1, *obs_shape)).to(device)
        self.actions = torch.zeros((batch_size, num_steps, 1)).to(device)
        self.rewards = torch.zeros((batch_size, num_steps, 1)).to(device)
        self.values = torch.zeros((batch_size, num_steps, 1)).to(device)
        self.dones = torch.zeros((batch_size, num_steps, 1)).to(device)
        self.action_log_probs = torch.zeros((batch_size, num_steps, 1)).to(device)

    def insert(self, b, step, o, a, r, v, d, alp):
        self.obs[b, step + 1] = torch.as_tensor(o)
        self.rewards[b, step] = torch.as_tensor(r)
        self.dones[b, step] = torch.as_tensor(d)
        self.actions[b, step] = a
        self.values[b, step] = v
        self.action_log_probs[b, step] = alp

    def insert_batch(self, step, o, a, r, v, d, alp):
        self.obs[:, step + 1] = o
        self.rewards[:, step] = r
        self.dones[:, step] = d
        self.actions[:, step] = a
        self.values[:, step] = v
        self.action_log_probs[:, step] = alp


class Runner:
    def __init__(self, env, task, summary_path, device, agent, actor_critic, num_steps, batch_size, discount, do_train, writer=None):
        self.env, self.task = env, task
        self.summary_path = summary_path
        dev = None if device is None else torch.device(device)
        self.device = torch.device('cpu') if dev is None else dev
        self.agent, self.actor_critic = agent, actor_critic
        self.num_steps, self.batch_size, self.discount, self.do_train = num_steps, batch_size, discount, do_train
        self.summary_writer = writer
        self.batch_counter = 0
        self.episode_counter = 0
        self.actor_critic.to(self.device)

    def _calculate_returns(self, next_value, rewards, dones):
        """next_value (b, 1), rewards, dones (b, n, 1) -> the discounted returns (b, n, 1)"""
        returns = torch.zeros((rewards.size(0), rewards.size(1) + 1, 1), dtype=rewards.dtype, device=rewards.device)
        returns[:, -1] = next_value
        for step in reversed(range(rewards.size(1))):
            returns[:, step] = returns[:, step + 1] * self.discount * (1 - dones[:, step]) + rewards[:, step]
        return returns[:, :-1]

    def _log_to_tb(self, log_dict, use_total_steps=True):
        if self.summary_writer is None:
            return
        counter = self.batch_counter * self.num_steps * self.batch_size if use_total_steps else self.batch_counter
        for key, value in log_dict.items():
            self.summary_writer.add_scalar(key, value, counter)

    def reset(self, frame_buffer=False):
        """a new configuration and one step with action 0, as the reference starts every trajectory -> (frame, state).
        frame_buffer: the image arm's start -- the task's frame buffer zeroed and filled by four steps with action 0 -> what the last
        step_frame_buffer returns (buffer, state, reward, done)"""
        self.env.reset()
        if frame_buffer:
            self.task.frame_buffer[:] = 0.
            for _ in range(3):
                self.task.step_frame_buffer(0)
            return self.task.step_frame_buffer(0)
        img, state, _, _ = self.task.step(0)
        return img, state

    def run_batch(self):
        raise NotImplementedError


class PPORunner(Runner):
    def __init__(self, env, task, summary_path=None, device=None, agent=None, actor_critic=None, num_steps=128, batch_size=32, discount=0.99,
                 do_train=True, writer=None, device_envs=None):
        """device_envs: False keeps the environments on the host while the policy is updated on `device`; None / True: they live where
        the policy lives.  self.fused_widths (an attribute, mcts_stove.FUSED_WIDTHS = (32,) by default): the state-code lengths of the
        learned model at which the model-based arm's one-launch collection is offered, as BatchedMCTSHandler.fused_widths is for
        planning; 16 and 64 are switched on by assigning it"""
        super().__init__(env, task, summary_path, device, agent, actor_critic, num_steps, batch_size, discount, do_train, writer)
        from ..mcts.mcts_stove import FUSED_WIDTHS
        self.fused_widths = FUSED_WIDTHS
        self.env_device = self.device if device_envs is None or device_envs else torch.device('cpu')
        if self.env_device.type == 'cuda' and self.device.type != 'cuda':
            raise ValueError('device_envs needs the policy on a GPU')

    # ------------------------------------------------------------------------------------------------ the collection
    def start_batch(self, batch_size, frame_buffer=False):
        """batch_size start states drawn one after the other from the runner's environment -> a host BatchedAvoidance holding them.
        frame_buffer: the image arm's start states, drawn with env.reset() only -- the four warm-up steps that fill the frame buffer
        belong to the collection (collect_images), which steps the whole batch through them together"""
        xs, vs = [], []
        for _ in range(batch_size):
            if frame_buffer:
                self.env.reset()
            else:
                self.reset()
            xs.append(np.array(self.env.x, dtype=np.float64))
            vs.append(np.array(self.env.v, dtype=np.float64))
        batch = BatchedAvoidance.from_tasks([self.task] * batch_size)
        batch.x, batch.v = np.stack(xs), np.stack(vs)
        return batch

    def fused_serves(self):
        return self.env_device.type == 'cuda' and self.actor_critic.kernel_shape() is not None

    def collect(self, batch_size, num_steps, fused=None, u=None):
        """-> (dict of obs (B, S + 1, 4N), rewards, values, logp, returns (B, S), next_value (B,) float32, actions (B, S), status (B,),
        as tensors on the runner's device; the stepped BatchedAvoidance).  u: the (B, S) float32 table of uniforms, drawn from numpy's
        global stream when None."""
        if u is None:
            u = np.random.random_sample((batch_size, num_steps)).astype(np.float32).clip(max=np.float32(1) - np.float32(2) ** -24)
        u = np.ascontiguousarray(u, dtype=np.float32)
        if u.shape != (batch_size, num_steps):
            raise ValueError('u is %s, the batch needs %s' % (u.shape, (batch_size, num_steps)))
        if fused and not self.fused_serves():
            raise ValueError('fused=True needs a device batch and a policy stove_ppo_collect serves: Policy(base="control") on 1 .. 6 '
                             'objects with a head of width 1 .. 128 and nine actions')
        batch = self.start_batch(batch_size)
        if self.env_device.type != 'cuda':
            if self.actor_critic.kernel_shape() is None:
                raise ValueError('the host collection restates Policy(base="control"); this policy is another one')
            out = _collect.PolicyForest.from_policy(self.actor_critic).collect(batch, u, self.discount)
            return {k: torch.from_numpy(a).to(self.device) for k, a in out.items()}, batch
        batch.to(self.device)
        ut = torch.from_numpy(u).to(self.device)
        if fused or (fused is None and self.fused_serves()):
            from .. import ops
            _, H, deep = self.actor_critic.kernel_shape()
            out = ops.ppo_collect(batch.x, batch.v, batch.r, batch.m, self.actor_critic.flat_params(), ut, H, deep, batch.granularity, batch.hw,
                                  batch.t, batch.friction, batch.action_force, batch.drift, self.discount)
            return out, batch
        return self._collect_composed(batch, ut), batch

    @torch.no_grad()
    def _collect_composed(self, batch, u):
        B, S = u.shape
        storage = BatchStorage(B, S, (4 * batch.n,), self.device)
        flat = lambda: batch.state().reshape(B, -1).float()
        storage.obs[:, 0] = flat()
        for step in range(S):
            value, action, logp = self.actor_critic.act(storage.obs[:, step], u=u[:, step])
            _, reward = batch.step(action, render=False)
            storage.insert_batch(step, flat(), action.reshape(B, 1), reward.reshape(B, 1), value, 0., logp)
        next_value = self.actor_critic.get_value(storage.obs[:, -1])
        returns = self._calculate_returns(next_value, storage.rewards, storage.dones)
        return {'obs': storage.obs, 'actions': storage.actions[:, :, 0].to(torch.int32), 'rewards': storage.rewards[:, :, 0],
                'values': storage.values[:, :, 0], 'logp': storage.action_log_probs[:, :, 0], 'next_value': next_value[:, 0],
                'returns': returns[:, :, 0], 'status': batch.status}

    # ------------------------------------------------------------------------------------------------ a batch
    def run_batch_states(self, fused=None, u=None):
        """collect batch_size trajectories of num_steps, then one PPO update on them -> the collection (see collect)"""
        out, batch = self.collect(self.batch_size, self.num_steps, fused, u)
        if bool(out['status'].any()):
            bad = torch.nonzero(out['status']).reshape(-1).tolist()
            raise RuntimeError('the policy put out a non-finite value or logit in environments %s (status %s)'
                               % (bad, out['status'][bad].tolist()))
        self.last_batch = batch
        three = lambda a: a.unsqueeze(-1)
        values, returns = three(out['values']), three(out['returns'])
        adv_targ = (returns - values).detach()
        losses = self._train_ppo(out['obs'][:, :-1], three(out['actions']).long(), returns, values, three(out['logp']), adv_targ)
        self._log_to_tb({'/losses/value_loss': losses[0], '/losses/action_loss': losses[1], '/losses/entropy': losses[2],
                         '/info/rewards': float(out['rewards'].mean())})
        self.batch_counter += 1
        return out

    # ------------------------------------------------------------------------------------------------ the arm on images
    WARM = 4          # steps with action 0 that fill the frame buffer before step 0 (the reference's reset(frame_buffer=True))

    def fused_serves_images(self):
        """whether stove_ppo_collect_images serves this runner: device environments that render 32 x 32 colour frames for a policy
        with an image_kernel_shape() on the task's number of stacked frames"""
        shape = self.actor_critic.image_kernel_shape()
        return (self.env_device.type == 'cuda' and shape is not None and self.env.res == 32 and not self.task.greyscale
                and self.task.get_framebuffer_shape()[2] == 3 * shape[0])

    def collect_images(self, batch_size, num_steps, fused=None, u=None):
        """-> (dict of frames (B, F + S, C, res, res) -- C = 3, or 1 with a greyscale task --, rewards, values, logp, returns (B, S),
        next_value (B,) float32, actions (B, S), status (B,), as tensors on the runner's device; the stepped BatchedAvoidance).  The
        observation of step s is frames[:, s:s + F], channels frame by frame, oldest first.  u: the (B, S) float32 table of uniforms,
        drawn from numpy's global stream when None.  fused: None -- one launch (stove_ppo_collect_images) where fused_serves_images
        holds, else the composed loop; True -- the launch or a ValueError; False -- the loop, on the device or on the host."""
        if u is None:
            u = np.random.random_sample((batch_size, num_steps)).astype(np.float32).clip(max=np.float32(1) - np.float32(2) ** -24)
        u = np.ascontiguousarray(u, dtype=np.float32)
        if u.shape != (batch_size, num_steps):
            raise ValueError('u is %s, the batch needs %s' % (u.shape, (batch_size, num_steps)))
        serves = self.fused_serves_images()
        if fused and not serves:
            raise ValueError('fused=True needs a device batch of 32 x 32 colour frames and a policy stove_ppo_collect_images serves: '
                             'Policy((32, 32, 3 F), 9) without use_grid, F in 1 .. 4, with a head of width 1 .. 512 and nine actions')
        batch = self.start_batch(batch_size, frame_buffer=True)
        ut = torch.from_numpy(u).to(self.device)
        if self.env_device.type == 'cuda':
            batch.to(self.device)
        if fused or (fused is None and serves):
            from .. import ops
            F, H, deep = self.actor_critic.image_kernel_shape()
            out = ops.ppo_collect_images(batch.x, batch.v, batch.r, batch.m, self.actor_critic.flat_image_params(), ut, F, H, deep, self.WARM,
                                         batch.granularity, batch.hw, batch.t, batch.friction, batch.action_force, batch.use_colors,
                                         batch.drift, self.discount)
            return out, batch
        return self._collect_images_composed(batch, ut), batch

    def _frame_rows(self, frames):
        """a step's rendered frames (B, 3, res, res), numpy or tensor -> float32 rows (B, C, res, res) on the runner's device"""
        rows = torch.as_tensor(frames).to(self.device)
        if self.task.greyscale:
            weights = torch.tensor([0.3, 0.59, 0.11], dtype=torch.float64, device=self.device).reshape(1, 3, 1, 1)
            rows = (rows.double() * weights).sum(1, keepdim=True).float()
        return rows

    @staticmethod
    def stacked(frames, F):
        """frames (B, R, C, res, res) -> the R - F + 1 windows (B, R - F + 1, F C, res, res): channel f C + c, oldest frame first"""
        B, R, C, h, w = frames.shape
        return frames.unfold(1, F, 1).permute(0, 1, 5, 2, 3, 4).reshape(B, R - F + 1, F * C, h, w)

    @torch.no_grad()
    def _collect_images_composed(self, batch, u):
        B, S = u.shape
        C = self.task.frame_channels
        F = self.task.get_framebuffer_shape()[2] // C
        frames = torch.zeros((B, F + S, C, batch.res, batch.res), device=self.device)
        zero = np.zeros(B, dtype=np.int64)
        for w in range(self.WARM):
            img, _ = batch.step(zero, render=F - self.WARM + w >= 0)
            if img is not None:
                frames[:, F - self.WARM + w] = self._frame_rows(img)
        storage = BatchStorage(B, S, (), self.device)
        window = lambda s: frames[:, s:s + F].reshape(B, F * C, batch.res, batch.res)
        for step in range(S):
            value, action, logp = self.actor_critic.act(window(step), u=u[:, step])
            img, reward = batch.step(action if batch.device is not None else action.cpu().numpy(), render=True)
            frames[:, F + step] = self._frame_rows(img)
            storage.rewards[:, step] = torch.as_tensor(reward).to(self.device).reshape(B, 1)
            storage.actions[:, step], storage.values[:, step], storage.action_log_probs[:, step] = action.reshape(B, 1), value, logp
        next_value = self.actor_critic.get_value(window(S))
        returns = self._calculate_returns(next_value, storage.rewards, storage.dones)
        return {'frames': frames, 'actions': storage.actions[:, :, 0].to(torch.int32), 'rewards': storage.rewards[:, :, 0],
                'values': storage.values[:, :, 0], 'logp': storage.action_log_probs[:, :, 0], 'next_value': next_value[:, 0],
                'returns': returns[:, :, 0], 'status': torch.zeros(B, dtype=torch.int32, device=self.device)}

    def run_batch(self, fused=None, u=None):
        """One batch of the image arm (reference runners.py: PPORunner.run_batch): collect batch_size trajectories of num_steps on rendered
        frames, then one PPO update on the stacked observations (B S, F C, res, res) -- with a fused_images agent on the frames themselves,
        no stacked observation built -> the collection (see collect_images) with 'losses'"""
        out, batch = self.collect_images(self.batch_size, self.num_steps, fused, u)
        if bool(out['status'].any()):
            bad = torch.nonzero(out['status']).reshape(-1).tolist()
            raise RuntimeError('the policy put out a non-finite value or logit in environments %s (status %s)'
                               % (bad, out['status'][bad].tolist()))
        self.last_batch = batch
        F = out['frames'].shape[1] - self.num_steps
        three = lambda a: a.unsqueeze(-1)
        values, returns = three(out['values']), three(out['returns'])
        adv_targ = (returns - values).detach()
        if getattr(self.agent, 'fused_images', False):          # (the windows are read where the collection wrote them)
            out['losses'] = self.agent.update_windows(out['frames'], self.num_steps, out['actions'], out['returns'], out['values'], out['logp'],
                                                      adv_targ)
        else:
            obs = self.stacked(out['frames'], F)[:, :-1]
            out['losses'] = self._train_ppo(obs, three(out['actions']).long(), returns, values, three(out['logp']), adv_targ)
        self._log_to_tb({'/losses/value_loss': out['losses'][0], '/losses/action_loss': out['losses'][1], '/losses/entropy': out['losses'][2],
                         '/info/rewards': float(out['rewards'].mean())})
        self.batch_counter += 1
        return out

    def _test_actorcritic_images(self, batch_size, num_steps, fused=None, u=None):
        """the mean reward of a fresh collection on images, without an update"""
        out, _ = self.collect_images(batch_size, num_steps, fused, u)
        return float(out['rewards'].mean())

    # ------------------------------------------------------------------------------------------------ the model-based arm
    def fused_serves_model(self, state_model):
        """whether stove_ppo_collect_model[_cl] serves this policy on `state_model`: a device, a policy with a kernel_shape(), a float32
        action-conditioned model of a state-code length in self.fused_widths with nine actions on the policy's 1 .. 6 objects"""
        from ..mcts.mcts_stove import BatchedMCTSHandler
        c, shape = state_model.c, self.actor_critic.kernel_shape()
        return (self.device.type == 'cuda' and shape is not None and not BatchedMCTSHandler._fused_unserved(state_model, self.fused_widths)
                and bool(c.action_conditioned) and c.action_space == 9 and shape[0] == c.num_obj)

    def collect_model(self, state_model, z0, apps, fused=None, u=None):
        """S = num_steps imagined steps from the model states z0 (B, N, 18) with appearances apps (B, N, app_dim) or None -> dict of
        z_pred (B, S, N, 18), obs (B, S + 1, 4N), rewards, values, logp, returns (B, S), next_value (B,) float32, actions (B, S),
        status (B,) on the runner's device (states cl/2 + 2 wide on a model of another state-code length).  u: the (B, S) float32
        table of uniforms, drawn from numpy's global stream when None."""
        B, S = z0.shape[0], self.num_steps
        if u is None:
            u = np.random.random_sample((B, S)).astype(np.float32).clip(max=np.float32(1) - np.float32(2) ** -24)
        u = np.ascontiguousarray(u, dtype=np.float32)
        if u.shape != (B, S):
            raise ValueError('u is %s, the batch needs %s' % (u.shape, (B, S)))
        serves = self.fused_serves_model(state_model)
        if fused and not serves:
            cl = state_model.c.cl
            why = '' if cl in self.fused_widths else ' (this model has cl = %d; runner.fused_widths offers 16 and 64)' % cl
            raise ValueError('fused=True needs the policy and a float32 action-conditioned model of a state-code length in fused_widths = %s '
                             'with nine actions on a GPU, and Policy(base="control") on the model\'s 1 .. 6 objects with a head of width '
                             '1 .. 128%s' % (tuple(self.fused_widths), why))
        ut = torch.from_numpy(u).to(self.device)
        z0 = z0.to(self.device).float().contiguous()
        apps = None if apps is None else apps.to(self.device).float().contiguous()
        if not (fused or (fused is None and serves)):
            return self._collect_model_composed(state_model, z0, apps, ut)
        from .. import ops
        from ..mcts.mcts_stove import BatchedMCTSHandler
        _, H, deep = self.actor_critic.kernel_shape()
        dyn = state_model.dyn
        with torch.no_grad():
            emb_w, emb_b, gnn, rh = BatchedMCTSHandler._fused_weights(state_model)
            return ops.ppo_collect_model(z0, apps, self.actor_critic.flat_params(), emb_w, emb_b, gnn, rh, ut, H, deep, 2, dyn.use_elu,
                                         dyn.loop_consts(), self.env.hw, self.discount)

    def _observe_model(self, z):
        """model states (B, N, 18) -> the policy's rows (B, 4N): positions and velocities in the environment's units (reference
        runners.py:241-243)"""
        phys = z[:, :, 2:6].clone()
        phys[:, :, :2] = ((phys[:, :, :2] + 1) / 2) * self.env.hw
        phys[:, :, 2:] = phys[:, :, 2:] / 2 * self.env.hw
        return phys.reshape(z.shape[0], -1)

    @torch.no_grad()
    def _collect_model_composed(self, state_model, z0, apps, u):
        B, S = u.shape
        n_actions = self.task.get_action_space()
        storage = BatchStorage(B, S, (4 * z0.shape[1],), self.device)
        state, states = z0, []
        storage.obs[:, 0] = self._observe_model(state)
        for step in range(S):
            value, action, logp = self.actor_critic.act(storage.obs[:, step], u=u[:, step])
            one_hot = torch.nn.functional.one_hot(action.long(), n_actions).unsqueeze(1).float()
            z_pred, r = state_model.rollout(state, 1, actions=one_hot, appearance=apps)
            state = z_pred[:, 0]
            states.append(state)
            storage.insert_batch(step, self._observe_model(state), action.reshape(B, 1), (r[:, 0] - 1).reshape(B, 1), value, 0., logp)
        next_value = self.actor_critic.get_value(storage.obs[:, -1])
        returns = self._calculate_returns(next_value, storage.rewards, storage.dones)
        z_pred = torch.stack(states, 1) if states else z0.new_zeros((B, 0) + tuple(z0.shape[1:]))
        return {'z_pred': z_pred, 'obs': storage.obs, 'actions': storage.actions[:, :, 0].to(torch.int32), 'rewards': storage.rewards[:, :, 0],
                'values': storage.values[:, :, 0], 'logp': storage.action_log_probs[:, :, 0], 'next_value': next_value[:, 0],
                'returns': returns[:, :, 0], 'status': torch.zeros(B, dtype=torch.int32, device=self.device)}

    def run_pretrained_batch(self, state_model, encoded_states, apps, fused=None, u=None):
        """One batch of the model-based arm (reference runners.py: run_pretrained_batch): batch_size start states drawn from the encoded
        ones, num_steps steps imagined on `state_model` under the policy with the reward head's rewards, one PPO update on them, then
        the policy's mean reward over 16 x 32 steps of the real environment.  fused: None -- one launch (stove_ppo_collect_model)
        where fused_serves_model holds, else the composed loop; True -- the launch or a ValueError; False -- the loop: per step one
        batched Policy.act, one Stove.rollout of one step, one insert.  -> the collection (see collect_model) with 'test_reward'."""
        randints = torch.randint(0, len(encoded_states) - 1, (self.batch_size,)).long()
        z0 = encoded_states[randints.to(encoded_states.device)].clone()
        app0 = None if apps is None else apps[randints.to(apps.device)].clone()
        out = self.collect_model(state_model, z0, app0, fused, u)
        if bool(out['status'].any()):
            bad = torch.nonzero(out['status']).reshape(-1).tolist()
            raise RuntimeError('the policy put out a non-finite value or logit in trajectories %s (status %s)'
                               % (bad, out['status'][bad].tolist()))
        three = lambda a: a.unsqueeze(-1)
        values, returns = three(out['values']), three(out['returns'])
        adv_targ = (returns - values).detach()
        losses = self._train_ppo(out['obs'][:, :-1], three(out['actions']).long(), returns, values, three(out['logp']), adv_targ)
        out['losses'] = losses
        out['test_reward'] = self._test_actorcritic(16, 32)
        self._log_to_tb({'/losses/value_loss': losses[0], '/losses/action_loss': losses[1], '/losses/entropy': losses[2],
                         '/info/test_reward': out['test_reward']})
        self.batch_counter += 1
        return out

    def _test_actorcritic(self, batch_size, num_steps, fused=None, u=None):
        """the mean reward of a fresh collection, without an update"""
        out, _ = self.collect(batch_size, num_steps, fused, u)
        return float(out['rewards'].mean())

    def _train_ppo(self, obs, actions, returns, values, action_log_probs, adv_targ):
        flat = lambda a: a.reshape((-1, *a.size()[2:]))
        return self.agent.update(flat(obs), flat(actions), flat(returns), flat(values), flat(action_log_probs), flat(adv_targ))
