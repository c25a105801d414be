"""What the control arm's tests share: building and running the sanitized host drivers of tests/abi/, the one parser of
include/stove_hip.h, and guarded device buffers for the GPU tests."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_FLAGS = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off', '-Wall', '-Werror']


def build_driver(tmp_path_factory, name):
    """tests/abi/<name>.cpp as a stand-alone program under the sanitizers -> its path (skips without a host compiler)"""
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp(name) / name)
    r = subprocess.run([cxx, *DRIVER_FLAGS, '-o', exe, os.path.join(ROOT, 'tests', 'abi', name + '.cpp')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_driver(exe, tmp_path, ints, scalars, arrays, outputs):
    """`exe run IN OUT`.  IN: `ints` as int32, `scalars` as one array of their dtype (a list: float64), then `arrays` as they are;
    OUT cut by `outputs` = [(key, shape, dtype)], every byte of it -> {key: array}"""
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as fh:
        fh.write(np.asarray(ints, dtype=np.int32).tobytes())
        fh.write((scalars if isinstance(scalars, np.ndarray) else np.asarray(scalars, dtype=np.float64)).tobytes())
        for a in arrays:
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, 'run', src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr                     # (a sanitizer report ends the driver with a non-zero status)
    raw = open(dst, 'rb').read()
    out, pos = {}, 0
    for key, shape, dt in outputs:
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[key] = np.frombuffer(raw[pos:pos + n], dtype=dt).reshape(shape)
        pos += n
    assert pos == len(raw)
    return out


def run_modes(exe, modes, env=None):
    """the driver's checking modes (validate, status, corrupt): each ends with status 0 and no failure"""
    for mode in modes:
        r = subprocess.run([exe, mode], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert '0 failure(s)' in r.stdout


def header_decls():
    """{name: (return type, [parameter text])} of every stove_* function include/stove_hip.h declares, comments stripped"""
    text = open(os.path.join(ROOT, 'include', 'stove_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    decls = {}
    for ret, name, params in re.findall(r'^\s*([A-Za-z_][\w \t]*?[\w*])\s*\b(stove_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;', text, flags=re.M | re.S):
        params = [' '.join(p.split()) for p in params.split(',')]
        decls[name] = (' '.join(ret.split()).replace(' *', '*'), [] if params == ['void'] else params)
    return decls


def header_decl(name):
    """(return type, [parameter text]) of `name` as include/stove_hip.h declares it"""
    decls = header_decls()
    assert name in decls, name + ' is not declared in include/stove_hip.h'
    return decls[name]


def guarded(values, fill, guard=64, device='cuda:0'):
    """a contiguous device copy of `values` with `guard` elements of `fill` in front of and behind it -> (view, whole buffer)"""
    flat = values.reshape(-1)
    buf = torch.full((flat.numel() + 2 * guard,), fill, dtype=values.dtype)
    buf[guard:guard + flat.numel()] = flat
    buf = buf.to(device)
    return buf[guard:guard + flat.numel()].view(values.shape), buf


def margins_intact(buffers, guard=64):
    """the margins of guarded() buffers still hold their fill: NaN in floating-point buffers, -77 in integer ones.
    guard: the margins' width, or {key: width}"""
    for k, buf in buffers.items():
        g = guard[k] if isinstance(guard, dict) else guard
        for edge in (buf[:g].cpu(), buf[-g:].cpu()):
            assert bool(torch.isnan(edge).all()) if buf.dtype.is_floating_point else bool((edge == -77).all()), k
