"""Float64 restatement of the pixel-space evaluation (numpy only, no torch ops): the composed paste of Supair.reconstruct_from_z per
channel at run-time geometry, the per-frame squared error, and the constant-velocity baseline of the pixel-error evaluation.

Layout, as the model's code has it: a frame plane is W rows of H columns (config.width, config.height), a patch plane pw rows of ph
columns; the transform's x (sx, z[2]) runs along the columns, its y (sy, z[3]) along the rows."""
import numpy as np


def base_grid(n, align_corners):
    """affine_grid's normalised coordinates of n pixels."""
    i = np.arange(n, dtype=np.float64)
    if n == 1:
        return np.zeros(1)
    return 2.0 * i / (n - 1) - 1.0 if align_corners else (2.0 * i + 1.0) / n - 1.0


def unnormalise(g, n, align_corners):
    """grid_sample's source index of a normalised coordinate over n source pixels."""
    return (g + 1.0) * 0.5 * (n - 1) if align_corners else ((g + 1.0) * n - 1.0) * 0.5


def _taps(s, n):
    """s (..,) source indices -> (i0, i1, w0, w1) with the weights of taps outside [0, n) zeroed and their indices clipped."""
    f = np.floor(s)
    t = s - f
    i0 = f.astype(np.int64)
    i1 = i0 + 1
    w0 = np.where((i0 >= 0) & (i0 < n), 1.0 - t, 0.0)
    w1 = np.where((i1 >= 0) & (i1 < n), t, 0.0)
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), w0, w1


def paste(patch, z, W, H, align_corners):
    """patch (C, pw, ph), z (4,) = [sx, sy, x, y] -> (C, W, H): grid_sample of the patch through [[1/sx, 0, -x/sx], [0, 1/sy, -y/sy]],
    bilinear, zero padding."""
    patch = np.asarray(patch, dtype=np.float64)
    sx, sy, x, y = (float(v) for v in z[:4])
    _, pw, ph = patch.shape
    gx = base_grid(H, align_corners) / sx - x / sx                # per column
    gy = base_grid(W, align_corners) / sy - y / sy                # per row
    c0, c1, wc0, wc1 = _taps(unnormalise(gx, ph, align_corners), ph)
    r0, r1, wr0, wr1 = _taps(unnormalise(gy, pw, align_corners), pw)
    out = np.zeros((patch.shape[0], W, H))
    for ri, wr in ((r0, wr0), (r1, wr1)):
        for ci, wc in ((c0, wc0), (c1, wc1)):
            out += patch[:, ri][:, :, ci] * (wr[:, None] * wc[None, :])[None]
    return out


def patch_row(f, k, n_obj, frames_per_patch):
    return 0 if frames_per_patch == 0 else (f // frames_per_patch) * n_obj + k


def render(bg, patches, frames_per_patch, z, n_obj, geom):
    """bg (C*W*H,), patches (., C*pw*ph), z (nf*n_obj, 4), geom = (C, W, H, pw, ph, align_corners) -> frames (nf, C*W*H) float64;
    patch row of (frame f, object k) = (f // frames_per_patch) * n_obj + k, row 0 for all when frames_per_patch == 0."""
    C, W, H, pw, ph, ac = geom
    bg = np.asarray(bg, dtype=np.float64).reshape(C, W, H)
    patches = np.asarray(patches, dtype=np.float64).reshape(-1, C, pw, ph)
    z = np.asarray(z, dtype=np.float64).reshape(-1, n_obj, 4)
    out = np.empty((z.shape[0], C, W, H))
    for f in range(z.shape[0]):
        acc = bg.copy()
        for k in range(n_obj):
            acc = acc + paste(patches[patch_row(f, k, n_obj, frames_per_patch)], z[f, k], W, H, bool(ac))
        out[f] = np.clip(acc, 0.0, 1.0)
    return out.reshape(z.shape[0], -1)


def sqerr(frames, truth):
    """(nf, P), (nf, P) -> (nf,) sum over a frame's pixels of (frame - truth)^2, float64."""
    d = np.asarray(frames, dtype=np.float64).reshape(len(frames), -1) - np.asarray(truth, dtype=np.float64).reshape(len(frames), -1)
    return (d * d).sum(1)


def mse_per_step(frames, truth):
    """(n, T, ...), (n, T, ...) -> (T,) mean over sequences and pixels (channels included) of the squared error."""
    f, t = np.asarray(frames, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return ((t - f) ** 2).reshape(f.shape[0], f.shape[1], -1).mean((0, 2))


def linear_baseline(z_last, num):
    """Constant-velocity extrapolation of the last inferred state: z_last (n, o, >=6) = [sx, sy, x, y, vx, vy, rest..] -> (n, num, o, D):
    sizes, velocities and the rest held, positions x + v * t for t = 1..num."""
    z_last = np.asarray(z_last, dtype=np.float64)
    t = np.arange(1, num + 1, dtype=np.float64)[None, :, None, None]
    rep = np.repeat(z_last[:, None], num, axis=1)
    rep[..., 2:4] = z_last[:, None, :, 2:4] + z_last[:, None, :, 4:6] * t
    return rep


def linear_clamp(z_seq, coord_lim):
    """The evaluation's position clamp for the baseline: positions to +-0.8 (coord_lim == 10) or +-0.9, the velocity columns dropped:
    (.., D) -> (.., D - 2) = [sx, sy, clamp(x, y), rest..]."""
    z_seq = np.asarray(z_seq, dtype=np.float64)
    lim = 0.8 if coord_lim == 10 else 0.9
    return np.concatenate([z_seq[..., :2], np.clip(z_seq[..., 2:4], -lim, lim), z_seq[..., 6:]], -1)


def draw_case(seed, n_frames, n_obj, geom, frames_per_patch):
    """Inputs of one kernel case: z scale in [0.1, 0.8], aspect in [0.5, 1.5], position in [-1.1, 1.1], bg in [0, 1], patches in
    [-0.5, 1.5], truth in [0, 1] -> dict of float32 arrays (objects hang over every edge, glimpses are magnified and minified, both
    clamp bounds are hit)."""
    C, W, H, pw, ph, _ = geom
    rng = np.random.RandomState(seed)
    rows = 1 if frames_per_patch == 0 else ((n_frames + frames_per_patch - 1) // frames_per_patch) * n_obj
    z = np.empty((n_frames * n_obj, 4))
    z[:, 0] = rng.uniform(0.1, 0.8, len(z))
    z[:, 1] = z[:, 0] * rng.uniform(0.5, 1.5, len(z))
    z[:, 2:] = rng.uniform(-1.1, 1.1, (len(z), 2))
    return dict(bg=rng.uniform(0.0, 1.0, C * W * H).astype(np.float32),
                patches=rng.uniform(-0.5, 1.5, (rows, C * pw * ph)).astype(np.float32),
                z=z.astype(np.float32),
                truth=rng.uniform(0.0, 1.0, (n_frames, C * W * H)).astype(np.float32))


# ---- the kernel cases shared by the CPU and the GPU tests
PIX_TOL = 2e-5                 # the project's pixel bar (tests/test_gpu_render.py): fp32 bilinear sums on values in [0, 1]
GEOMS = ((1, 32, 32, 10, 10), (3, 12, 20, 8, 12), (3, 50, 50, 10, 10))
OBJECTS, FRAMES, PER = (1, 3, 8), (1, 3, 65), (0, 1, 5)


MAX_CLAMPED = 0.60            # at most this share of a case's pixels may sit on a clamp bound (the comparison is not one of constants)


def clamped_share(frames):
    return float(((frames == 0.0) | (frames == 1.0)).mean())


_CASES = {}
REDRAWS = {}                 # (geom5, align_corners, n_obj, n_frames, per) -> draws rejected before the one that is used


def kernel_cases(geom5, align_corners):
    """every (n_obj, n_frames, frames_per_patch) of one geometry and sampling convention -> [(n_obj, n_frames, per, geom, inputs, ref)],
    ref = render() of the inputs in float64, computed once per process.  A draw whose frames are clamped over more than MAX_CLAMPED of
    their pixels is drawn again with the next seed (one frame of eight objects can be mostly saturated); the condition is on the inputs
    alone."""
    key = (tuple(geom5), bool(align_corners))
    if key not in _CASES:
        geom = key[0] + (key[1],)
        out = []
        for n_obj in OBJECTS:
            for nf in FRAMES:
                for per in PER:
                    seed = 1000 * GEOMS.index(key[0]) + 500 * int(key[1]) + 100 * n_obj + 7 * nf + per
                    for attempt in range(20):
                        inp = draw_case(seed + 10000 * attempt, nf, n_obj, geom, per)
                        ref = render(inp['bg'], inp['patches'], per, inp['z'], n_obj, geom)
                        if clamped_share(ref) <= MAX_CLAMPED:
                            break
                    else:
                        raise RuntimeError('no draw of %s within the clamped share' % ((n_obj, nf, per, geom),))
                    REDRAWS[key + (n_obj, nf, per)] = attempt
                    out.append((n_obj, nf, per, geom, inp, ref))
        _CASES[key] = out
    return _CASES[key]


def sqerr_bound(frames64, truth, tol):
    """What |sqerr - sqerr64| may be when every pixel is within tol of its float64 value and the sum is taken in float32:
    2 tol sum|frame64 - truth| + P tol^2 + 1e-6 sqerr64, per frame."""
    f = np.asarray(frames64, dtype=np.float64).reshape(len(frames64), -1)
    t = np.asarray(truth, dtype=np.float64).reshape(len(frames64), -1)
    return 2.0 * tol * np.abs(f - t).sum(1) + f.shape[1] * tol * tol + 1e-6 * ((f - t) ** 2).sum(1)


def matched_position_error(pos, true, fit_frames):
    """pos, true (n, T, o, 2): per sequence the object permutation with the smallest mean distance over the first fit_frames frames,
    then the mean distance per time step over sequences and objects -> ((T,), chosen permutation index per sequence)."""
    import itertools
    pos, true = np.asarray(pos, dtype=np.float64), np.asarray(true, dtype=np.float64)
    perms = list(itertools.permutations(range(pos.shape[2])))
    errs = np.stack([np.sqrt(((true[:, :fit_frames] - pos[:, :fit_frames][:, :, list(p)]) ** 2).sum(-1)).mean((1, 2)) for p in perms], 1)
    best = errs.argmin(1)
    matched = np.stack([pos[i][:, list(perms[j])] for i, j in enumerate(best)], 0)
    return np.sqrt(((true - matched) ** 2).sum(-1)).mean((0, 2)), best
