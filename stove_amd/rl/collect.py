"""The PPO arm's collection on states on the host: `PolicyForest`, the numpy restatement of stove_amd/csrc/ppo_policy.h that the
one-launch kernel (stove_ppo_collect) and the CPU driver are held to, as EnvForest is for the search.  Vectorised over the
environments with ELEMENTWISE float32 / float64 ufuncs only, in the operation order of the header: a neuron is one float32 sum that
starts at its bias and adds w[k] * x[k] for k ascending, multiply and add rounded separately, so everything but the two library
calls of the draw (exp, log) is reproduced bit for bit.

The draw inverts the cumulative distribution at a uniform u[b][s] in [0, 1) from a table the caller draws up front (`uniforms`).  The
reference draws with `Categorical.sample()`, whose stream of torch's generator depends on the device and on the batch shape: that
stream cannot be reproduced and is not.  The distribution drawn from is the same.

`ImageForest` is the same for the arm on images: the numpy restatement of stove_amd/csrc/ppo_image.h (stove_ppo_collect_images), the
CNN policy on a window of rendered frames with every convolution output one serial float32 sum as well."""
import numpy as np

ACTIONS = 9
BASE0, BASE1 = 128, 32
OK, NON_FINITE = 0, 3
KEYS = ('obs', 'actions', 'rewards', 'values', 'logp', 'next_value', 'returns', 'status')
MODEL_STATE_WIDTHS = (10, 18, 34)          # cl/2 + 2 of the models the model-based arm's kernels serve (cl = 16, 32, 64)


def uniforms(B, S, seed):
    """the (B, S) float32 table of one collection, in [0, 1)"""
    return np.random.RandomState(seed).random_sample((B, S)).astype(np.float32).clip(max=np.float32(1) - np.float32(2) ** -24)


def layer_shapes(N, H, deep):
    """[(in, out)] of the image's layers: ppo_policy.h's width_in / width_out"""
    return [(4 * N, BASE0), (BASE0, BASE1), (BASE1, H)] + ([(H, H), (H, H)] if deep else []) + [(H, 1 + ACTIONS)]


def param_floats(N, H, deep):
    return sum((k + 1) * j for k, j in layer_shapes(N, H, deep))


def _dense(h, layers):
    """(K, in) float32 through Linear + ReLU layers [(wT (in, out), bias)], the last one without ReLU: a neuron is one float32 sum from
    its bias, k ascending"""
    with np.errstate(invalid='ignore', over='ignore'):
        for l, (wT, bias) in enumerate(layers):
            acc = np.repeat(bias[None, :], h.shape[0], axis=0)
            for k in range(wT.shape[0]):
                acc = acc + wT[k][None, :] * h[:, k, None]
            h = np.where(acc < 0, np.float32(0), acc) if l != len(layers) - 1 else acc
    assert h.dtype == np.float32
    return h


class PolicyForest:
    """params: the float32 image of Policy.flat_params() for (N, H, deep)."""

    def __init__(self, params, N, H, deep):
        params = np.ascontiguousarray(np.asarray(params, dtype=np.float32)).reshape(-1)
        if not 1 <= N <= 6 or not 1 <= H <= 128:
            raise ValueError('PolicyForest holds 1 .. 6 objects and head widths 1 .. 128, not N = %d, H = %d' % (N, H))
        if params.size != param_floats(N, H, deep):
            raise ValueError('the image of (N, H, deep) = (%d, %d, %s) has %d floats, not %d' % (N, H, bool(deep), param_floats(N, H, deep),
                                                                                             params.size))
        self.N, self.H, self.deep = int(N), int(H), bool(deep)
        self.layers, at = [], 0
        for k, j in layer_shapes(N, H, deep):
            self.layers.append((params[at:at + k * j].reshape(k, j), params[at + k * j:at + (k + 1) * j]))
            at += (k + 1) * j

    @classmethod
    def from_policy(cls, policy):
        shape = policy.kernel_shape()
        if shape is None:
            raise ValueError('PolicyForest restates Policy(base="control") with nine actions')
        return cls(policy.flat_params().cpu().numpy(), *shape)

    # ------------------------------------------------------------------------------------------------ the header, function by function
    @staticmethod
    def observe(x, v):
        """(K, N, 2) float64 twice -> (K, 4N) float32"""
        return np.concatenate([x, v], axis=2).reshape(x.shape[0], -1).astype(np.float32)

    def forward(self, obs):
        """(K, 4N) float32 -> heads (K, 10) float32: column 0 the value, columns 1 .. 9 the logits"""
        return _dense(obs, self.layers)

    @staticmethod
    def draw(logits, u):
        """(K, 9) float32, (K,) float32 -> actions (K,) int32, logp (K,) float32, margin (K,) float64"""
        d = logits - logits.max(axis=1, keepdims=True)
        c = np.zeros(d.shape, dtype=np.float64)
        run = np.zeros(d.shape[0], dtype=np.float64)
        for a in range(ACTIONS):
            run = run + np.exp(d[:, a].astype(np.float64))
            c[:, a] = run
        thr = u.astype(np.float64) * run
        above = c > thr[:, None]
        actions = np.where(above.any(axis=1), above.argmax(axis=1), ACTIONS - 1).astype(np.int32)
        margin = (np.abs(c - thr[:, None]) / run[:, None]).min(axis=1)
        chosen = d[np.arange(d.shape[0]), actions].astype(np.float64)
        return actions, (chosen - np.log(run)).astype(np.float32), margin

    @staticmethod
    def discounted(rewards, next_value, discount):
        """(K, S), (K,) float32 -> returns (K, S) float32: returns[s] = returns[s + 1] * discount + rewards[s]"""
        g = np.float32(discount)
        out = np.zeros(rewards.shape, dtype=np.float32)
        run = next_value.astype(np.float32)
        for s in range(rewards.shape[1] - 1, -1, -1):
            run = run * g + rewards[:, s]
            out[:, s] = run
        return out

    # ------------------------------------------------------------------------------------------------ the model-based arm's policy half
    @staticmethod
    def observe_model(z, hw):
        """(K, N, 18) float32 model states (10 or 34 wide for a cl = 16 / 64 model: only columns 2 .. 5 are read) -> (K, 4N) float32:
        ppo_policy.h's observe_model, positions (z + 1) / 2 * hw, velocities z / 2 * hw, every operation rounded to float32 on its
        own, hw rounded once (reference runners.py:241-243)"""
        z = np.asarray(z, dtype=np.float32)
        hw, one, two = np.float32(hw), np.float32(1), np.float32(2)
        with np.errstate(invalid='ignore', over='ignore'):
            pos = (z[:, :, 2:4] + one) / two * hw
            vel = z[:, :, 4:6] / two * hw
        obs = np.concatenate([pos, vel], axis=2).reshape(z.shape[0], -1)
        assert obs.dtype == np.float32
        return obs

    def decide_model(self, z, hw, u):
        """One decision per model state: z (K, N, 18) float32, u (K,) float32 uniforms -> (obs (K, 4N), values (K,), actions (K,) int32,
        logp (K,) float32, margin (K,) float64): the specification of what stove_ppo_collect_model does between two steps of the model.
        States of a cl = 16 / 64 model, (K, N, 10) / (K, N, 34), are read the same way (stove_ppo_collect_model_cl)."""
        z = np.asarray(z, dtype=np.float32)
        if z.ndim != 3 or z.shape[1] != self.N or z.shape[2] not in MODEL_STATE_WIDTHS:
            raise ValueError('z is %s, the policy reads (K, %d, 18) (or 10 / 34 wide)' % (z.shape, self.N))
        u = np.asarray(u)
        if u.dtype != np.float32 or u.shape != (z.shape[0],):
            raise ValueError('u must be a float32 vector of %d uniforms' % z.shape[0])
        obs = self.observe_model(z, hw)
        heads = self.forward(obs)
        actions, logp, margin = self.draw(heads[:, 1:], u)
        return obs, heads[:, 0], actions, logp, margin

    # ------------------------------------------------------------------------------------------------ the collection
    def collect(self, batch, u, discount=0.95):
        """S = u.shape[1] steps of the host BatchedAvoidance `batch` (stepped in place) -> dict of obs (B, S + 1, 4N), rewards, values,
        logp, returns (B, S), next_value (B,) float32, actions (B, S), status (B,) int32; rows never written are zero.  self.margin (B,):
        the smallest decision margin min_a |c_a - u c_8| / c_8 of each environment's draws (inf without a draw)."""
        if batch.device is not None:
            raise ValueError('PolicyForest collects on a host BatchedAvoidance; a device batch goes through ops.ppo_collect')
        if batch.n != self.N:
            raise ValueError('the policy reads %d objects, the batch holds %d' % (self.N, batch.n))
        u = np.asarray(u)
        B, N = batch.M, self.N
        if u.dtype != np.float32 or u.ndim != 2 or u.shape[0] != B:
            raise ValueError('u must be a float32 table (%d, S)' % B)
        S = u.shape[1]
        out = {'obs': np.zeros((B, S + 1, 4 * N), np.float32), 'actions': np.zeros((B, S), np.int32), 'rewards': np.zeros((B, S), np.float32),
               'values': np.zeros((B, S), np.float32), 'logp': np.zeros((B, S), np.float32), 'next_value': np.zeros(B, np.float32),
               'returns': np.zeros((B, S), np.float32), 'status': np.zeros(B, np.int32)}
        self.margin = np.full(B, np.inf)
        going = np.ones(B, dtype=bool)
        for t in range(S + 1):
            rows = np.flatnonzero(going)
            if rows.size == 0:
                break
            obs = self.observe(batch.x[rows], batch.v[rows])
            heads = self.forward(obs)
            fine = np.isfinite(heads).all(axis=1)
            out['status'][rows[~fine]] = NON_FINITE
            going[rows[~fine]] = False
            rows, obs, heads = rows[fine], obs[fine], heads[fine]
            if rows.size == 0:
                break
            out['obs'][rows, t] = obs
            if t == S:
                out['next_value'][rows] = heads[:, 0]
                out['returns'][rows] = self.discounted(out['rewards'][rows], heads[:, 0], discount)
                break
            actions, logp, margin = self.draw(heads[:, 1:], u[rows, t])
            x, v = batch.x[rows], batch.v[rows]
            hits = batch._step_rows(x, v, batch.r[rows], batch.m[rows], actions.astype(np.int64))
            batch.x[rows], batch.v[rows] = x, v
            out['values'][rows, t], out['actions'][rows, t], out['logp'][rows, t] = heads[:, 0], actions, logp
            out['rewards'][rows, t] = (-hits).astype(np.float32)
            self.margin[rows] = np.minimum(self.margin[rows], margin)
        return out


# ------------------------------------------------------------------------------------------------ the arm on images
RES, MAPS, SIDE1, SIDE2, FLAT = 32, 32, 15, 7, 32 * 7 * 7
MAX_FRAMES, MAX_IMAGE_HIDDEN = 4, 512
IMAGE_KEYS = ('frames', 'actions', 'rewards', 'values', 'logp', 'next_value', 'returns', 'status')


def image_layer_shapes(F, H, deep):
    """[(in, out)] of the image policy's layers: ppo_image.h's width_in / width_out"""
    return [(48 * F, MAPS), (9 * MAPS, MAPS), (FLAT, H)] + ([(H, H), (H, H)] if deep else []) + [(H, 1 + ACTIONS)]


def image_param_floats(F, H, deep):
    """ppo_image.h's param_floats; 0 outside F in 1 .. 4, H in 1 .. 512, as stove_ppo_image_param_floats"""
    if not 1 <= F <= MAX_FRAMES or not 1 <= H <= MAX_IMAGE_HIDDEN:
        return 0
    return sum((k + 1) * j for k, j in image_layer_shapes(F, H, deep))


class ImageForest:
    """The numpy restatement of stove_amd/csrc/ppo_image.h, which the one-launch kernel (stove_ppo_collect_images) and the CPU driver are
    held to, as PolicyForest is for states.  params: the float32 image of Policy.flat_image_params() for (F, H, deep).  Frames are
    (3, 32, 32) float32 rows in the layout BatchedAvoidance.step renders; a window is the last F of them, oldest first."""

    def __init__(self, params, F, H, deep):
        params = np.ascontiguousarray(np.asarray(params, dtype=np.float32)).reshape(-1)
        if not 1 <= F <= MAX_FRAMES or not 1 <= H <= MAX_IMAGE_HIDDEN:
            raise ValueError('ImageForest holds windows of 1 .. 4 frames and head widths 1 .. 512, not F = %d, H = %d' % (F, H))
        if params.size != image_param_floats(F, H, deep):
            raise ValueError('the image of (F, H, deep) = (%d, %d, %s) has %d floats, not %d'
                             % (F, H, bool(deep), image_param_floats(F, H, deep), params.size))
        self.F, self.H, self.deep = int(F), int(H), bool(deep)
        self.layers, at = [], 0
        for k, j in image_layer_shapes(F, H, deep):
            self.layers.append((params[at:at + k * j].reshape(k, j), params[at + k * j:at + (k + 1) * j]))
            at += (k + 1) * j

    @classmethod
    def from_policy(cls, policy):
        shape = policy.image_kernel_shape()
        if shape is None:
            raise ValueError('ImageForest restates Policy((32, 32, 3 F), 9) without use_grid, F in 1 .. 4, head width 1 .. 512')
        return cls(policy.flat_image_params().cpu().numpy(), *shape)

    # ------------------------------------------------------------------------------------------------ the header, function by function
    @staticmethod
    def _conv(x, wT, bias, kernel, side):
        """(K, C, s, s) float32 -> ReLU of the stride-2 convolution (K, 32, side, side): one float32 sum per output, from its bias,
        k = (c * kernel + ky) * kernel + kx ascending"""
        K, C = x.shape[:2]
        span = 2 * side - 1
        with np.errstate(invalid='ignore', over='ignore'):
            acc = np.repeat(np.repeat(np.repeat(bias[None, :, None, None], K, axis=0), side, axis=2), side, axis=3)
            k = 0
            for c in range(C):
                for ky in range(kernel):
                    for kx in range(kernel):
                        acc = acc + wT[k][None, :, None, None] * x[:, c, None, ky:ky + span:2, kx:kx + span:2]
                        k += 1
            out = np.where(acc < 0, np.float32(0), acc)
        assert out.dtype == np.float32
        return out

    def forward(self, window):
        """(K, F, 3, 32, 32) float32 frames, oldest first -> heads (K, 10) float32: column 0 the value, columns 1 .. 9 the logits"""
        window = np.asarray(window)
        if window.dtype != np.float32 or window.ndim != 5 or window.shape[1:] != (self.F, 3, RES, RES):
            raise ValueError('the window must be float32 (K, %d, 3, 32, 32)' % self.F)
        with np.errstate(invalid='ignore'):
            x = (window / np.float32(255.0)).reshape(window.shape[0], 3 * self.F, RES, RES)
        c1 = self._conv(x, *self.layers[0], 4, SIDE1)
        c2 = self._conv(c1, *self.layers[1], 3, SIDE2)
        return _dense(c2.reshape(c2.shape[0], FLAT), self.layers[2:])

    def decide(self, frames_window, u):
        """One decision per window: (K, F, 3, 32, 32) float32, u (K,) float32 uniforms -> (values (K,), actions (K,) int32, logp (K,)
        float32, margin (K,) float64).  self.heads (K, 10): the ten outputs behind them."""
        u = np.asarray(u)
        if u.dtype != np.float32 or u.shape != (np.asarray(frames_window).shape[0],):
            raise ValueError('u must be a float32 vector of one uniform per window')
        self.heads = self.forward(frames_window)
        with np.errstate(invalid='ignore'):
            actions, logp, margin = PolicyForest.draw(self.heads[:, 1:], u)
        return self.heads[:, 0], actions, logp, margin

    # ------------------------------------------------------------------------------------------------ the collection
    def collect(self, batch, u, discount=0.95, warm=4):
        """`warm` steps with action 0, then S = u.shape[1] steps of the host BatchedAvoidance `batch` (stepped in place) -> dict of frames
        (B, F + S, 3, 32, 32), rewards, values, logp, returns (B, S), next_value (B,) float32, actions (B, S), status (B,) int32; rows
        never written are zero.  Step s reads frames[:, s:s + F].  self.margin (B,): the smallest decision margin of each environment's
        draws (inf without a draw)."""
        if batch.device is not None:
            raise ValueError('ImageForest collects on a host BatchedAvoidance; a device batch goes through ops.ppo_collect_images')
        if batch.res != RES:
            raise ValueError('the image policy reads 32 x 32 frames, the batch renders %d x %d' % (batch.res, batch.res))
        u = np.asarray(u)
        B, F = batch.M, self.F
        if u.dtype != np.float32 or u.ndim != 2 or u.shape[0] != B:
            raise ValueError('u must be a float32 table (%d, S)' % B)
        if warm < 1:
            raise ValueError('the collection starts with at least one warm-up step')
        S = u.shape[1]
        out = {'frames': np.zeros((B, F + S, 3, RES, RES), np.float32), 'actions': np.zeros((B, S), np.int32),
               'rewards': np.zeros((B, S), np.float32), 'values': np.zeros((B, S), np.float32), 'logp': np.zeros((B, S), np.float32),
               'next_value': np.zeros(B, np.float32), 'returns': np.zeros((B, S), np.float32), 'status': np.zeros(B, np.int32)}
        self.margin = np.full(B, np.inf)
        frames = np.zeros((B, F + S, 3, RES, RES), np.float32)          # (what the ring holds; `out` gets a row once it counts as written)
        with np.errstate(invalid='ignore', over='ignore'):
            for w in range(warm):
                batch._step_rows(batch.x, batch.v, batch.r, batch.m, np.zeros(B, dtype=np.int64))
                if F - warm + w >= 0:
                    frames[:, F - warm + w] = batch._draw(batch.x, batch.r)
        going = np.ones(B, dtype=bool)
        for t in range(S + 1):
            rows = np.flatnonzero(going)
            if rows.size == 0:
                break
            heads = self.forward(frames[rows, t:t + F])
            fine = np.isfinite(heads).all(axis=1)
            out['status'][rows[~fine]] = NON_FINITE
            going[rows[~fine]] = False
            rows, heads = rows[fine], heads[fine]
            if rows.size == 0:
                break
            if t == 0:
                out['frames'][rows, :F] = frames[rows, :F]
            if t == S:
                out['next_value'][rows] = heads[:, 0]
                out['returns'][rows] = PolicyForest.discounted(out['rewards'][rows], heads[:, 0], discount)
                break
            actions, logp, margin = PolicyForest.draw(heads[:, 1:], u[rows, t])
            x, v = batch.x[rows], batch.v[rows]
            hits = batch._step_rows(x, v, batch.r[rows], batch.m[rows], actions.astype(np.int64))
            batch.x[rows], batch.v[rows] = x, v
            frames[rows, F + t] = out['frames'][rows, F + t] = batch._draw(x, batch.r[rows])
            out['values'][rows, t], out['actions'][rows, t], out['logp'][rows, t] = heads[:, 0], actions, logp
            out['rewards'][rows, t] = (-hits).astype(np.float32)
            self.margin[rows] = np.minimum(self.margin[rows], margin)
        return out
