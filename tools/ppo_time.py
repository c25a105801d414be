"""Time one PPO batch on states, piece by piece, on this tree (writes profiles/ppo_collect.json):

    python tools/ppo_time.py [--reps 5] [--out profiles/ppo_collect.json]

Per batch of 32 x 128 and 256 x 128 steps (N = 3, H = 64, main_rl's environment settings), wall-clock with a device synchronisation
at either end, the median of --reps runs after one warm-up:
  start_ms      drawing the batch's start states on the host (reset + one step each; common to every variant below)
  fused_ms      the one-launch collection (ops.ppo_collect), the image built from the policy included
  composed_ms   the composed device collection: per step one batched policy.act and one stove_env_step
  host_loop_ms  the reference's shape: environment after environment, per step a one-row policy.act on the device, a .cpu() and a
                numpy AvoidanceTask.step (--reps 1 for this one: it is slow by construction)
  update_ms     PPOAgent.update on the collected batch (4 epochs x 32 mini-batches, torch autograd + Adam)

    python tools/ppo_time.py --update [--reps 5] [--update-out profiles/ppo_update.json]

times the update alone, both ways in this one process on the same collected batch (writes profiles/ppo_update.json):
  torch_update_ms   PPOAgent.update as above (the code path of fused=None, unchanged by the fused one)
  fused_update_ms   PPOAgent(fused=True).update: the permutations, their upload, the image, one stove_ppo_update launch, the image
                    written back into the policy, and the one read of the losses and the status
  fused_launch_ms   ops.ppo_update alone on prepared tensors

    python tools/ppo_time.py --model [--reps 5] [--model-out profiles/ppo_model.json]

times the model-based arm's collection (PPORunner.collect_model) of 32 x 128 and 256 x 128 imagined steps on an untrained, seeded
action-conditioned cl = 32 model of three objects with appearances (the arithmetic does not depend on the weights), both ways in this
one process from the same start states and uniforms (writes profiles/ppo_model.json):
  composed_ms   the composed loop: per step one batched Policy.act, one Stove.rollout of one step (embedding, rollout and reward-head
                launches) and one insert -- calls that all predate the one-launch collection, which is what makes it the baseline
  fused_ms      the one-launch collection (ops.ppo_collect_model), the policy's and the model's images built included
  fused_launch_ms   ops.ppo_collect_model alone on prepared images
and per imagined step of a trajectory, fused_launch_ms / 128, as step_us.  --cl 16 / 64: the same on a model of that state-code length
(ops.ppo_collect_model on stove_ppo_collect_model_cl), the runner's fused_widths switched on for it; the result goes under the key
cl16 / cl64 of profiles/ppo_model_cl.json, beside what the file already holds.

    python tools/ppo_time.py --images [--reps 5] [--images-hidden 512] [--images-out profiles/ppo_image.json]

times the arm on images (PPORunner.collect_images) at 32 x 128 and 256 x 128 steps with N = 3, F = 4 stacked frames and head width
512, both ways in this one process from the same start states and uniforms (writes profiles/ppo_image.json):
  start_ms          drawing the batch's start states on the host (env.reset() each)
  fused_launch_ms   ops.ppo_collect_images alone on a prepared image, the four warm-up steps included; step_us: that per step of the 132
  fused_ms          collect_images(fused=True): the start states, their upload and the image included
  composed_ms       the composed device loop: per step one batched Policy.act on the window and one stove_env_step with its frame
  update_ms         for context: PPOAgent.update on the collected batch (4 epochs x 32 mini-batches, torch autograd + Adam), once

    python tools/ppo_time.py --images-update [--reps 5] [--images-update-out profiles/ppo_image_update.json]

times the update of the image policy (N = 3, F = 4, head widths 512 and 64, 4 epochs x 32 mini-batches) at 32 x 128 and 256 x 128, three
ways in this one process on the same collected batch (writes profiles/ppo_image_update.json):
  torch_update_ms     what PPORunner.run_batch does with a torch agent: the stacked windows built from the frames, then PPOAgent.update
  update_windows_ms   PPOAgent(fused_images=True).update_windows on the frames: the permutations, their upload, the image, the chain of
                      launches of stove_ppo_update_images, the image written back and the one read of the losses and the status
  launch_ms           ops.ppo_update_images alone on prepared tensors; step_us: that per optimiser step of the 128"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stove_amd import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ppo_collect.json'))
    ap.add_argument('--update', action='store_true', help='time the update alone: torch against the one-launch update')
    ap.add_argument('--update-out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ppo_update.json'))
    ap.add_argument('--model', action='store_true', help='time the model-based collection: the composed loop against the one launch')
    ap.add_argument('--model-out', default=None, help='default: profiles/ppo_model.json, at --cl 16 / 64 profiles/ppo_model_cl.json')
    ap.add_argument('--cl', type=int, default=32, choices=(16, 32, 64), help='state-code length of the model of --model')
    ap.add_argument('--images', action='store_true', help='time the collection on images: the composed loop against the one launch')
    ap.add_argument('--images-hidden', type=int, default=512, help='head width of the image policy (main_rl\'s default 512)')
    ap.add_argument('--images-out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ppo_image.json'))
    ap.add_argument('--images-update', action='store_true', help='time the update of the image policy: torch against the device chain')
    ap.add_argument('--images-update-out',
                    default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ppo_image_update.json'))
    args = ap.parse_args()
    if args.model_out is None:
        args.model_out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                      'ppo_model.json' if args.cl == 32 else 'ppo_model_cl.json')
    build.build_library()
    import numpy as np
    import torch
    from stove_amd import ops
    from stove_amd.envs import envs
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.rl_model import Policy
    from stove_amd.rl.runners import PPORunner

    dev = 'cuda:0'
    sync = torch.cuda.synchronize

    def timed(fn, reps):
        fn()
        times = []
        for _ in range(reps):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times)

    result = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'policy': {'N': 3, 'H': 64, 'deep': False}, 'batches': {}}
    if args.model:
        from stove_amd.mcts.mcts_stove import BatchedMCTSHandler
        from stove_amd.video_prediction.config import StoveConfig
        from stove_amd.video_prediction.stove import Stove
        cfg = StoveConfig()
        cfg.num_obj, cfg.width, cfg.height, cfg.debug = 3, 32, 32, True
        cfg.device, cfg.dtype, cfg.random_seed = torch.device(dev), torch.float32, 42
        cfg.action_conditioned, cfg.action_space, cfg.debug_core_appearance = True, 9, True
        cl = args.cl
        if cl != 32:
            cfg.cl, cfg.transition_lik_std = cl, [0.01] * (cl // 2)
        torch.manual_seed(0)
        model = Stove(cfg).to(dev)
        for p in model.parameters():
            p.requires_grad_(False)
        result['model'] = {'cl': cl, 'num_obj': 3, 'app_dim': 3, 'action_space': 9}
        for B, S in ((32, 128), (256, 128)):
            torch.manual_seed(0)
            np.random.seed(0)
            env = envs.BillardsEnv(n=3, granularity=2, seed=0)
            task = envs.AvoidanceTask(env, action_force=.3)
            policy = Policy(12, 9, hidden_size=64, base='control')
            agent = PPOAgent(policy, .1, 4, 32, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
            runner = PPORunner(env, task, None, dev, agent, policy, num_steps=S, batch_size=B, discount=.95)
            if cl != 32:
                runner.fused_widths = (cl,)
            u = np.random.random_sample((B, S)).astype(np.float32)
            rs = np.random.RandomState(1)
            z = np.concatenate([np.full((B, 3, 2), 0.1), rs.uniform(-0.7, 0.7, (B, 3, 2)), rs.uniform(-0.1, 0.1, (B, 3, 2)),
                                rs.uniform(-0.5, 0.5, (B, 3, cl // 2 - 4))], axis=2).astype(np.float32)
            z0 = torch.from_numpy(z).to(dev)
            apps = torch.from_numpy(rs.uniform(0, 1, (B, 3, 3)).astype(np.float32)).to(dev)
            assert runner.fused_serves_model(model)
            row = {'composed_ms': timed(lambda: runner.collect_model(model, z0, apps, fused=False, u=u), args.reps),
                   'fused_ms': timed(lambda: runner.collect_model(model, z0, apps, fused=True, u=u), args.reps)}
            with torch.no_grad():
                emb_w, emb_b, gnn, rh = BatchedMCTSHandler._fused_weights(model)
            image, ut = policy.flat_params(), torch.from_numpy(u).to(dev)
            launch = lambda out=None: ops.ppo_collect_model(z0, apps, image, emb_w, emb_b, gnn, rh, ut, 64, False, 2, model.dyn.use_elu,
                                                            model.dyn.loop_consts(), env.hw, .95, out=out)
            outs = launch()
            row['fused_launch_ms'] = timed(lambda: launch(outs), args.reps)
            row['step_us'] = row['fused_launch_ms'] * 1e3 / S
            row['fused_status_any'] = bool(outs['status'].any())
            composed = runner.collect_model(model, z0, apps, fused=False, u=u)
            row['actions_agree'] = float((composed['actions'] == outs['actions']).float().mean())
            result['batches']['%dx%d' % (B, S)] = row
            print('%dx%d' % (B, S), json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(args.model_out), exist_ok=True)
        if cl != 32:                                             # one file for the widths other than 32, a key per width
            whole = json.load(open(args.model_out)) if os.path.isfile(args.model_out) else {}
            whole['cl%d' % cl] = result
            result = whole
        with open(args.model_out, 'w') as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
        return
    if args.images_update:
        result['policy'] = {'F': 4, 'deep': False}
        result['update'] = {'epochs': 4, 'mini_batches': 32}
        for H in (512, 64):
            for B, S in ((32, 128), (256, 128)):
                torch.manual_seed(0)
                np.random.seed(0)
                env = envs.BillardsEnv(n=3, granularity=2, seed=0)
                task = envs.AvoidanceTask(env, num_stacked=4, action_force=.3)
                policy = Policy(task.get_framebuffer_shape(), 9, hidden_size=H, stacked_frames=4)
                agent = PPOAgent(policy, .1, 4, 32, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
                runner = PPORunner(env, task, None, dev, agent, policy, num_steps=S, batch_size=B, discount=.95)
                u = np.random.random_sample((B, S)).astype(np.float32)
                out, _ = runner.collect_images(B, S, fused=True, u=u)
                three = lambda a: a.unsqueeze(-1)
                flat = lambda a: a.reshape((-1, *a.size()[2:]))
                adv = out['returns'] - out['values']

                def torch_update():          # (what run_batch does without fused_images: the stacked windows are built per update)
                    obs = flat(runner.stacked(out['frames'], 4)[:, :-1])
                    return agent.update(obs, flat(three(out['actions']).long()), flat(three(out['returns'])), flat(three(out['values'])),
                                        flat(three(out['logp'])), flat(three(adv)))

                row = {'torch_update_ms': timed(torch_update, args.reps)}
                twin = Policy(task.get_framebuffer_shape(), 9, hidden_size=H, stacked_frames=4).to(dev)
                twin.load_state_dict(policy.state_dict())
                fused_agent = PPOAgent(twin, .1, 4, 32, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, fused_images=True)
                row['update_windows_ms'] = timed(lambda: fused_agent.update_windows(out['frames'], S, out['actions'], out['returns'], out['values'],
                                                                                    out['logp'], adv), args.reps)
                n = B * S
                image = twin.flat_image_params()
                m, v, step = torch.zeros_like(image), torch.zeros_like(image), torch.zeros(1, dtype=torch.int32, device=dev)
                perm = torch.stack([torch.randperm(n) for _ in range(4)]).to(device=dev, dtype=torch.int32)
                rows = [out['actions'].reshape(n)] + [t.reshape(n).contiguous() for t in (out['returns'], out['values'], out['logp'], adv)]
                launch = lambda o=None: ops.ppo_update_images(image, m, v, step, out['frames'], *rows, perm, 32, 4, H, False, .1, .5, .01, 2e-4, 1e-5,
                                                              40., steps_per_env=S, out=o)
                outs = launch()
                row['launch_ms'] = timed(lambda: launch(outs), args.reps)
                row['step_us'] = row['launch_ms'] * 1e3 / 128
                row['status'] = outs['status'].tolist()
                row['workspace_mb'] = ops._PPO_IMAGE_WS[(image.device, n, 32, 4, H, 0)].numel() * 4 / 2 ** 20
                result['batches']['h%d_%dx%d' % (H, B, S)] = row
                print('h%d_%dx%d' % (H, B, S), json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(args.images_update_out), exist_ok=True)
        with open(args.images_update_out, 'w') as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
        return
    if args.images:
        result['policy'] = {'F': 4, 'H': args.images_hidden, 'deep': False}
        for B, S in ((32, 128), (256, 128)):
            torch.manual_seed(0)
            np.random.seed(0)
            env = envs.BillardsEnv(n=3, granularity=2, seed=0)
            task = envs.AvoidanceTask(env, num_stacked=4, action_force=.3)
            policy = Policy(task.get_framebuffer_shape(), 9, hidden_size=args.images_hidden, stacked_frames=4)
            agent = PPOAgent(policy, .1, 4, 32, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
            runner = PPORunner(env, task, None, dev, agent, policy, num_steps=S, batch_size=B, discount=.95)
            assert runner.fused_serves_images()
            u = np.random.random_sample((B, S)).astype(np.float32)
            ut = torch.from_numpy(u).to(dev)
            row = {'start_ms': timed(lambda: runner.start_batch(B, frame_buffer=True), args.reps)}
            start = runner.start_batch(B, frame_buffer=True).to(dev)
            x0, v0 = start.x.clone(), start.v.clone()
            image = policy.flat_image_params()

            def rewind():
                start.x.copy_(x0)
                start.v.copy_(v0)

            def launch(out=None):
                rewind()
                return ops.ppo_collect_images(start.x, start.v, start.r, start.m, image, ut, 4, args.images_hidden, False, runner.WARM,
                                              start.granularity, start.hw, start.t, start.friction, start.action_force, start.use_colors,
                                              start.drift, .95, out=out)

            def composed():
                rewind()
                return runner._collect_images_composed(start, ut)

            outs = launch()
            row['fused_launch_ms'] = timed(lambda: launch(outs), args.reps)
            row['step_us'] = row['fused_launch_ms'] * 1e3 / (S + runner.WARM)
            row['fused_ms'] = timed(lambda: runner.collect_images(B, S, fused=True, u=u), args.reps)
            row['composed_ms'] = timed(composed, args.reps)
            row['fused_status_any'] = bool(outs['status'].any())
            row['actions_agree'] = float((composed()['actions'] == launch()['actions']).float().mean())
            out = launch()
            three = lambda a: a.unsqueeze(-1)
            flat = lambda a: a.reshape((-1, *a.size()[2:]))
            batch = [flat(runner.stacked(out['frames'], 4)[:, :-1]), flat(three(out['actions']).long()), flat(three(out['returns'])),
                     flat(three(out['values'])), flat(three(out['logp'])), flat(three(out['returns'] - out['values']))]
            row['update_ms'] = timed(lambda: agent.update(*batch), 1)
            result['batches']['%dx%d' % (B, S)] = row
            print('%dx%d' % (B, S), json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(args.images_out), exist_ok=True)
        with open(args.images_out, 'w') as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
        return
    for B, S in ((32, 128), (256, 128)):
        torch.manual_seed(0)
        np.random.seed(0)
        env = envs.BillardsEnv(n=3, granularity=2, seed=0)
        task = envs.AvoidanceTask(env, action_force=.3)
        policy = Policy(12, 9, hidden_size=64, base='control')
        agent = PPOAgent(policy, .1, 4, 32, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
        runner = PPORunner(env, task, None, dev, agent, policy, num_steps=S, batch_size=B, discount=.95)
        u = np.random.random_sample((B, S)).astype(np.float32)
        ut = torch.from_numpy(u).to(dev)
        row = {'start_ms': timed(lambda: runner.start_batch(B), args.reps)}
        start = runner.start_batch(B).to(dev)
        x0, v0 = start.x.clone(), start.v.clone()

        def rewind():
            start.x.copy_(x0)
            start.v.copy_(v0)

        def fused():
            rewind()
            return ops.ppo_collect(start.x, start.v, start.r, start.m, policy.flat_params(), ut, 64, False, start.granularity, start.hw, start.t,
                                   start.friction, start.action_force, start.drift, .95)

        def composed():
            rewind()
            return runner._collect_composed(start, ut)

        def host_loop():
            with torch.no_grad():
                for b in range(B):
                    _, state = runner.reset()
                    obs = torch.from_numpy(state.reshape(1, -1)).float().to(dev)
                    for s in range(S):
                        value, action, logp = policy.act(obs)
                        _, state, r, _ = task.step(int(action[0].cpu()))
                        obs = torch.from_numpy(state.reshape(1, -1)).float().to(dev)

        if not args.update:
            row['fused_ms'] = timed(fused, args.reps)
            row['composed_ms'] = timed(composed, args.reps)
            row['host_loop_ms'] = timed(host_loop, 1)
        out = fused()
        three = lambda a: a.unsqueeze(-1)
        flat = lambda a: a.reshape((-1, *a.size()[2:]))
        batch = [flat(out['obs'][:, :-1]), flat(three(out['actions']).long()), flat(three(out['returns'])), flat(three(out['values'])),
                 flat(three(out['logp'])), flat(three(out['returns'] - out['values']))]
        if args.update:
            row = {'torch_update_ms': timed(lambda: agent.update(*batch), args.reps)}
            twin = Policy(12, 9, hidden_size=64, base='control').to(dev)
            twin.load_state_dict(policy.state_dict())
            fused_agent = PPOAgent(twin, .1, 4, 32, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, fused=True)
            row['fused_update_ms'] = timed(lambda: fused_agent.update(*batch), args.reps)
            n = batch[0].shape[0]
            image = twin.flat_params()
            m, v, step = torch.zeros_like(image), torch.zeros_like(image), torch.zeros(1, dtype=torch.int32, device=dev)
            perm = torch.stack([torch.randperm(n) for _ in range(4)]).to(device=dev, dtype=torch.int32)
            rows = [batch[0].contiguous(), batch[1].reshape(n).to(torch.int32)] + [t.reshape(n).contiguous() for t in batch[2:]]
            outs = ops.ppo_update(image, m, v, step, *rows, perm, 32, 64, False, .1, .5, .01, 2e-4, 1e-5, 40.)
            row['fused_launch_ms'] = timed(lambda: ops.ppo_update(image, m, v, step, *rows, perm, 32, 64, False, .1, .5, .01, 2e-4, 1e-5, 40., out=outs),
                                           args.reps)
            row['fused_status'] = outs['status'].tolist()
        else:
            row['update_ms'] = timed(lambda: agent.update(*batch), max(1, args.reps // 2))
        result['batches']['%dx%d' % (B, S)] = row
        print('%dx%d' % (B, S), json.dumps(row), flush=True)
    path = args.update_out if args.update else args.out
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
