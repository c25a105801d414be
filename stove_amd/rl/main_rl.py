"""Train the PPO arms (counterpart of the reference's model/rl/main_rl.py): `parse_args` carries the reference's flags, `main` serves
`--use-states`, the model-free arm, and `--use-pretrained-model`, the model-based one, on the billiards environment under the
avoidance task.  `--device-envs` keeps the batch of environments on the GPU, where a batch of trajectories is one launch
(stove_ppo_collect); without it the collection runs on the host (collect.PolicyForest) and only the update uses the device.
`--use-pretrained-model` trains on trajectories imagined by the learned dynamics model restored from `--checkpoint DIR`, started
from the states that model infers on the recorded sequences of `--data PKL` (pretrained.load_and_encode; the reference hard-codes
both paths); on a GPU a batch of imagined trajectories is one launch (stove_ppo_collect_model) on a cl = 32 model, and on a cl = 16 or
64 model once `--fused-widths 16,32,64` offers it (stove_ppo_collect_model_cl; without the flag such a model takes the composed loop).
The real environment only scores the policy after each update.  `--use-images` is the model-free arm on rendered frames, the baseline the learned model is measured
against: the CNN policy on the task's frame buffer, a batch of trajectories in one launch with `--device-envs`
(stove_ppo_collect_images), else a composed loop of batched steps; its update is torch autograd, or with `--fused-update` one chain
of launches on the frames the collection wrote (stove_ppo_update_images).  The reference runs this arm when no
flag is given; here the flag is required and a bare call raises NotImplementedError.  The gym and distance-task variants are not part
of this package."""
import argparse
import json
import os

import numpy as np
import torch

from ..envs.envs import AvoidanceTask, BillardsEnv
from .agents import PPOAgent
from .rl_model import Policy
from .runners import PPORunner


def parse_args(args):
    parser = argparse.ArgumentParser(description='RL')
    parser.add_argument('--experiment_id', default='ppo', help='name of the experiment')
    parser.add_argument('--env', default='billards', help='environment to use: billards')
    parser.add_argument('--task', default='avoidance', help='task to learn if training: avoidance | maxdist | mindist')
    parser.add_argument('--seed', type=int, default=0, help='random seed')
    parser.add_argument('--lr', type=float, default=2e-4, help='learning rate')
    parser.add_argument('--clip-param', type=float, default=0.1, help='ppo clip parameter')
    parser.add_argument('--num-steps', type=int, default=128, help='number of forward steps in PPO')
    parser.add_argument('--batch-size', type=int, default=32, help='number of trajectories sampled per batch')
    parser.add_argument('--num-env-steps', type=int, default=10000000, help='number of total environment steps')
    parser.add_argument('--num-ppo-mb', type=int, default=32, help='number of batches for ppo')
    parser.add_argument('--num-ppo-epochs', type=int, default=4, help='number of epochs for ppo')
    parser.add_argument('--save-interval', type=int, default=100, help='save interval, one save per n batches')
    parser.add_argument('--value-loss-coef', type=float, default=0.5, help='value loss coefficient')
    parser.add_argument('--entropy-coef', type=float, default=0.01, help='entropy term coefficient')
    parser.add_argument('--eps', type=float, default=1e-5, help='Adam optimizer epsilon')
    parser.add_argument('--max-grad-norm', type=float, default=40, help='max norm of gradients')
    parser.add_argument('--summary-dir', type=str, default='./summary/', help='directory to save args (and summaries of a writer)')
    parser.add_argument('--model-dir', type=str, default='./models/', help='directory to save models')
    parser.add_argument('--hidden-size', type=int, default=512, help='hidden size in the policy head (image variant)')
    parser.add_argument('--gym', action='store_true', default=False, help='whether or not to use gym as environment')
    parser.add_argument('--use-states', action='store_true', default=False, help='use states instead of images when true')
    parser.add_argument('--use-deep-layers', action='store_true', default=False, help='use more linear layers in head')
    parser.add_argument('--num-balls', type=int, default=3, help='number of balls to simulate in the environment')
    parser.add_argument('--radius', type=float, default=1., help='radius of each ball in the environment')
    parser.add_argument('--gran', type=int, default=2, help='granularity of the simulation in the environment')
    parser.add_argument('--dt', type=float, default=1., help='dt of the simulation computed in each time step')
    parser.add_argument('--action-force', type=float, default=.3, help='action force of the task simulation')
    parser.add_argument('--num-stacked-frames', type=int, default=4, help='number of frames stacked as inputs')
    parser.add_argument('--use-grid', action='store_true', default=False, help='add grid information to the visual input')
    parser.add_argument('--use-pretrained-model', action='store_true', default=False, help='use the pretrained model as world model')
    parser.add_argument('--use-images', action='store_true', default=False,
                        help='the model-free arm on rendered frames (what the reference runs when no flag is given)')
    parser.add_argument('--device-envs', action='store_true', default=False,
                        help='keep the environments on the GPU: a batch of trajectories is one launch')
    parser.add_argument('--fused-update', action='store_true', default=False,
                        help='run the PPO update on the GPU without host round trips (needs the policy and the batch there)')
    parser.add_argument('--device', default=None, help='device of the policy (default: cuda when there is one)')
    parser.add_argument('--checkpoint', default=None, help='run directory of the trained dynamics model (--use-pretrained-model)')
    parser.add_argument('--data', default=None, help='pickle of recorded sequences with actions to start from (--use-pretrained-model)')
    parser.add_argument('--fused-widths', default=None, metavar='16,32,64', type=lambda v: tuple(int(w) for w in v.split(',')),
                        help='state-code lengths of the learned model at which the one-launch collection of imagined trajectories is '
                             'offered (--use-pretrained-model; default: 32 alone)')
    args = parser.parse_args(args)
    assert args.task in ['avoidance', 'maxdist', 'mindist']
    assert not (args.gym and args.use_states)
    assert not (args.gym and args.use_pretrained_model)
    assert not (args.use_states and args.use_pretrained_model)
    assert not (args.use_images and (args.use_states or args.use_pretrained_model or args.gym))
    if not args.gym:
        assert args.env in ['billards']
    return args


def save_args(args, path):
    with open(os.path.join(path, 'args.json'), 'w') as fp:
        json.dump(vars(args), fp, sort_keys=True, indent=4)


def load_model(checkpoint, data, device):
    """the trained action-conditioned Stove of run directory `checkpoint`, on `device`, in eval mode"""
    from ..main import restore_model
    model = restore_model(checkpoint, extras={'nolog': True, 'traindata': data, 'testdata': data}).to(device)
    for p in model.parameters():
        p.requires_grad_(False)
    return model.eval()


def build(args, writer=None):
    """-> (runner, actor_critic) for parsed `args`"""
    use_images = getattr(args, 'use_images', False)
    if not (args.use_states or args.use_pretrained_model or use_images) or args.gym or args.task != 'avoidance':
        raise NotImplementedError('this package trains the avoidance task on states (--use-states), on the learned model '
                                  '(--use-pretrained-model) or on rendered frames (--use-images; the reference runs those when no flag '
                                  'is given, here the flag is required); the gym and distance-task variants are not part of it')
    if args.use_pretrained_model and (args.checkpoint is None or args.data is None):
        raise ValueError('--use-pretrained-model needs --checkpoint DIR (the trained dynamics model) and --data PKL (its sequences)')
    device = args.device or ('cuda' if torch.cuda.is_available() else 'cpu')
    if args.fused_update and torch.device(device).type != 'cuda':
        raise ValueError('--fused-update needs a GPU')
    if use_images and args.fused_update and (args.use_grid or not 1 <= args.num_stacked_frames <= 4 or not 1 <= args.hidden_size <= 512):
        raise ValueError('--use-images --fused-update serves the policy without --use-grid on 1 .. 4 stacked frames with a head of width '
                         '1 .. 512 (stove_ppo_update_images)')
    env =BillardsEnv(n=args.num_balls, r=args.radius, granularity=args.gran, t=args.dt, seed=args.seed)
    task = AvoidanceTask(env, num_stacked=args.num_stacked_frames, action_force=args.action_force, greyscale=False)
    if use_images:
        actor_critic = Policy(task.get_framebuffer_shape(), task.get_action_space(), hidden_size=args.hidden_size,
                              stacked_frames=args.num_stacked_frames, use_grid=args.use_grid, use_deep_layers=args.use_deep_layers)
    else:
        shape = env.get_state_shape()
        actor_critic = Policy(shape[0] * shape[1], task.get_action_space(), hidden_size=64, base='control')
    agent = PPOAgent(actor_critic, args.clip_param, args.num_ppo_epochs, args.num_ppo_mb, args.value_loss_coef, args.entropy_coef, args.lr,
                     args.eps, args.max_grad_norm, fused=True if args.fused_update and not use_images else None,
                     fused_images=True if args.fused_update and use_images else None)
    if args.device_envs and torch.device(device).type != 'cuda':
        raise ValueError('--device-envs needs a GPU')
    runner = PPORunner(env=env, task=task, summary_path=os.path.join(args.summary_dir, args.experiment_id), device=device, agent=agent,
                       actor_critic=actor_critic, num_steps=args.num_steps, batch_size=args.batch_size, discount=0.95, writer=writer,
                       device_envs=bool(args.device_envs))
    if getattr(args, 'fused_widths', None) is not None:
        runner.fused_widths = tuple(args.fused_widths)
    return runner, actor_critic


def main(args, writer=None):
    args = parse_args(args)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    model_path = os.path.join(args.model_dir, args.experiment_id)
    summary_path = os.path.join(args.summary_dir, args.experiment_id)
    os.makedirs(model_path, exist_ok=True)
    os.makedirs(summary_path, exist_ok=True)
    save_args(args, summary_path)
    runner, actor_critic = build(args, writer)
    num_batches = int(args.num_env_steps) // args.num_steps // args.batch_size
    save = lambda i: torch.save(actor_critic.state_dict(), os.path.join(model_path, 'model' + str(i) + '.pt'))
    i = 0
    try:
        if args.use_pretrained_model:
            from .pretrained import load_and_encode
            state_model = load_model(args.checkpoint, args.data, runner.device)
            encoded, apps = load_and_encode(args.data, state_model, runner.device)          # (once per run, not once per batch)
        for i in range(num_batches):
            if args.use_pretrained_model:
                runner.run_pretrained_batch(state_model, encoded, apps)
            elif args.use_images:
                runner.run_batch()
            else:
                runner.run_batch_states()
            if i % args.save_interval == 0:
                save(i)
    except BaseException:
        save(i)
        raise
    if not os.path.isfile(os.path.join(model_path, 'model' + str(i) + '.pt')):
        save(i)
    return runner
