#!/usr/bin/env python
"""Pixel-space prediction error of trained runs (the command line of the reference's scripts/pixel_error.py; the evaluation itself is
Trainer.pixel_error, rendered and scored on the GPU).

    python tools/pixel_error.py -p EXPERIMENT_DIR/ [--linear] [--real-mpe] [--no-save] [--checkpoint NAME]

-p is one run folder (a folder whose name starts with 'run') or a folder whose run* sub-folders are evaluated in name order; a run that
cannot be restored or scored is reported at the end and does not stop the others.  Per run one row is
appended to <path>/test/pixel_errors.csv (mean squared pixel error per time step) and to <path>/test/states_pixel_errors.csv (matched
position error per time step), `linear_`-prefixed for the constant-velocity baseline: values as {:.6f}, comma separated, one line."""
import argparse
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def csv_row(values):
    """one run's row: every value with six decimals, commas, a newline"""
    return ','.join('{:.6f}'.format(float(v)) for v in values) + '\n'


def csv_names(linear):
    name = ('linear_' if linear else '') + 'pixel_errors.csv'
    return name, 'states_' + name


def find_runs(path):
    """the run folders under -p: `path` itself when it is one, else its run* sub-folders in name order"""
    path = os.path.normpath(path)
    if os.path.basename(path).startswith('run'):
        return [path]
    if not os.path.isdir(path):
        return []
    return [os.path.join(path, d) for d in sorted(os.listdir(path)) if d.startswith('run') and os.path.isdir(os.path.join(path, d))]


def append_rows(path, linear, mse, mse_states):
    save_dir = os.path.join(path, 'test')
    os.makedirs(save_dir, exist_ok=True)
    for name, values in zip(csv_names(linear), (mse, mse_states)):
        with open(os.path.join(save_dir, name), 'a') as f:
            f.write(csv_row(values))


def evaluate(restore, linear, real_mpe, checkpoint):
    from stove_amd.main import main as restore_trainer
    trainer = restore_trainer(restore=restore, extras={'nolog': True, 'checkpoint_path': os.path.join(restore, checkpoint)})
    c = trainer.c
    print(c.testdata)
    print(c.frame_step, c.num_visible, c.batch_size, c.skip)        # runs that are compared must agree on these
    res = trainer.pixel_error(linear=linear, real_mpe=real_mpe)
    return res['mse'].numpy(), res['mse_states'].numpy()


def main(script_args=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-p', '--path', type=str, required=True, help='a run folder, or a folder that holds run* folders')
    ap.add_argument('--linear', action='store_true', help='score the constant-velocity baseline instead of the dynamics model')
    ap.add_argument('--no-save', dest='no_save', action='store_true', help='print only, append nothing')
    ap.add_argument('--real-mpe', dest='real_mpe', action='store_true', help='render with the MPE patches of the first scored frame')
    ap.add_argument('--checkpoint', type=str, default='checkpoint', help='checkpoint file inside each run folder')
    args = ap.parse_args(script_args)
    runs = find_runs(args.path)
    if not runs:
        ap.error('%s is no run folder and holds none' % args.path)
    print('%d run(s): %s' % (len(runs), ', '.join(runs)))
    failed = {}
    for restore in runs:
        try:
            mse, mse_states = evaluate(restore, args.linear, args.real_mpe, args.checkpoint)
        except Exception:               # an unreadable run is reported below, the sweep goes on
            failed[restore] = traceback.format_exc(limit=3)
        else:
            print('mse', csv_row(mse), end='')
            print('mse_states', csv_row(mse_states), end='')
            if not args.no_save:
                append_rows(args.path, args.linear, mse, mse_states)
    for restore, why in failed.items():
        print('skipped %s:\n%s' % (restore, why), file=sys.stderr)
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
