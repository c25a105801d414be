"""The PPO arm's collection on states on the host: `PolicyForest`, the numpy restatement of stove_amd/csrc/ppo_policy.h that the
one-launch kernel (stove_ppo_collect) and the CPU driver are held to, as EnvForest is for the search.  Vectorised over the
environments with ELEMENTWISE float32 / float64 ufuncs only, in the operation order of the header: a neuron is one float32 sum that
starts at its bias and adds w[k] * x[k] for k ascending, multiply and add rounded separately, so everything but the two library
calls of the draw (exp, log) is reproduced bit for bit.

The draw inverts the cumulative distribution at a uniform u[b][s] in [0, 1) from a table the caller draws up front (`uniforms`).  The
reference draws with `Categorical.sample()`, whose stream of torch's generator depends on the device and on the batch shape: that
stream cannot be reproduced and is not.  The distribution drawn from is the same."""
import numpy as np

ACTIONS = 9
BASE0, BASE1 = 128, 32
OK, NON_FINITE = 0, 3
KEYS = ('obs', 'actions', 'rewards', 'values', 'logp', 'next_value', 'returns', 'status')


def uniforms(B, S, seed):
    """the (B, S) float32 table of one collection, in [0, 1)"""
    return np.random.RandomState(seed).random_sample((B, S)).astype(np.float32).clip(max=np.float32(1) - np.float32(2) ** -24)


def layer_shapes(N, H, deep):
    """[(in, out)] of the image's layers: ppo_policy.h's width_in / width_out"""
    return [(4 * N, BASE0), (BASE0, BASE1), (BASE1, H)] + ([(H, H), (H, H)] if deep else []) + [(H, 1 + ACTIONS)]


def param_floats(N, H, deep):
    return sum((k + 1) * j for k, j in layer_shapes(N, H, deep))


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
        h = obs
        with np.errstate(invalid='ignore', over='ignore'):
            for l, (wT, bias) in enumerate(self.layers):
                acc = np.repeat(bias[None, :], h.shape[0], axis=0)
                for k in range(wT.shape[0]):
                    acc = acc + wT[k][None, :] * h[:, k, None]
                h = np.where(acc < 0, np.float32(0), acc) if l != len(self.layers) - 1 else acc
        assert h.dtype == np.float32
        return h

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
        """(K, N, 18) float32 model states -> (K, 4N) float32: ppo_policy.h's observe_model, positions (z + 1) / 2 * hw, velocities
        z / 2 * hw, every operation rounded to float32 on its own, hw rounded once (reference runners.py:241-243)"""
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
        logp (K,) float32, margin (K,) float64): the specification of what stove_ppo_collect_model does between two steps of the model."""
        z = np.asarray(z, dtype=np.float32)
        if z.ndim != 3 or z.shape[1:] != (self.N, 18):
            raise ValueError('z is %s, the policy reads (K, %d, 18)' % (z.shape, self.N))
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
