"""The policy networks of the model-free PPO arm (counterpart of the reference's model/rl/rl_model.py): same constructor arguments,
same act / get_value / evaluate_actions, same state_dict keys, so a reference checkpoint loads.  Plain torch modules: they run on the
CPU and on a GPU.  `Policy(base='control')` -- SimpleControlBase under DiscreteActionHead -- is the network the one-launch collection
serves (stove_ppo_collect, csrc/ppo_policy.h): `flat_params()` writes the image that kernel reads.  `Policy((32, 32, 3 F), 9)` --
SimpleCNNBase without use_grid under the same head -- is the network of the arm on images (PPORunner.run_batch); the one-launch
collection on images serves it for F in 1 .. 4 and head widths up to 512 (stove_ppo_collect_images, csrc/ppo_image.h):
`flat_image_params()` writes that kernel's image.  With use_grid the composed loop of the runner collects instead."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class Base(nn.Module):
    def __init__(self, hidden_size):
        super().__init__()
        self.output_size = hidden_size

    def forward(self, inputs):
        raise NotImplementedError


class Head(nn.Module):
    def forward(self, inputs):
        raise NotImplementedError


class Flatten(nn.Module):
    def forward(self, input):
        return input.view(input.size(0), -1)


class SimpleCNNBase(Base):
    """two strided convolutions on stacked frames in [0, 255]; with use_grid two coordinate channels are appended"""

    def __init__(self, num_inputs, hidden_size=32 * 7 * 7, use_grid=False):
        super().__init__(hidden_size)
        self.use_grid = use_grid
        self.main = nn.Sequential(nn.Conv2d(num_inputs, 32, kernel_size=4, stride=2), nn.ReLU(),
                                  nn.Conv2d(32, 32, kernel_size=3, stride=2), nn.ReLU(), Flatten())

    def forward(self, inputs):
        inp = inputs / 255.
        if self.use_grid:
            ys = torch.linspace(-1, 1, inputs.size(-2), device=inputs.device)
            xs = torch.linspace(-1, 1, inputs.size(-1), device=inputs.device)
            xv, yv = torch.meshgrid(ys, xs, indexing='ij')
            grid = torch.stack((xv, yv)).unsqueeze(0).to(inp.dtype)
            inp = torch.cat([inp, grid.expand(inp.size(0), -1, -1, -1)], 1)
        return self.main(inp)


class SimpleControlBase(Base):
    """Linear(num_inputs, 128), ReLU, Linear(128, hidden_size), ReLU on a state vector"""
    WIDTH = 128

    def __init__(self, num_inputs, hidden_size=32):
        super().__init__(hidden_size)
        self.main = nn.Sequential(nn.Linear(num_inputs, self.WIDTH), nn.ReLU(), nn.Linear(self.WIDTH, hidden_size), nn.ReLU())

    def forward(self, inputs):
        return self.main(inputs)


class DiscreteActionHead(Head):
    """Linear(num_inputs, hidden_size), ReLU [, two more Linear(hidden_size, hidden_size) + ReLU with use_deep_layers], then the value
    (hidden_size -> 1) and the logits of a Categorical (hidden_size -> action_space).  `in_between` holds parameters either way."""

    def __init__(self, num_inputs, action_space, hidden_size, use_deep_layers=False):
        super().__init__()
        self.use_deep_layers = use_deep_layers
        self.main = nn.Linear(num_inputs, hidden_size)
        self.in_between = nn.Sequential(nn.Linear(hidden_size, hidden_size), nn.ReLU(), nn.Linear(hidden_size, hidden_size), nn.ReLU())
        self.values_head = nn.Linear(hidden_size, 1)
        self.actor_head = nn.Linear(hidden_size, action_space)

    def features(self, inputs):
        x = F.relu(self.main(inputs))
        return self.in_between(x) if self.use_deep_layers else x

    def forward(self, inputs):
        x = self.features(inputs)
        return self.values_head(x), torch.distributions.Categorical(logits=self.actor_head(x))


class Policy(nn.Module):
    """base None: SimpleCNNBase on obs_shape (res, res, channels); base 'control': SimpleControlBase on obs_shape inputs."""

    def __init__(self, obs_shape, action_space, hidden_size=512, base=None, head=None, stacked_frames=4, use_grid=False,
                 use_deep_layers=False):
        super().__init__()
        self.stacked_frames = stacked_frames
        self.use_grid = use_grid
        if head is not None:
            raise NotImplementedError
        if base is None:
            self.base = SimpleCNNBase(obs_shape[2] + 2 if use_grid else obs_shape[2], use_grid=use_grid)
        elif base == 'control':
            self.base = SimpleControlBase(obs_shape)
        else:
            raise NotImplementedError
        self.head = DiscreteActionHead(self.base.output_size, action_space, hidden_size=hidden_size, use_deep_layers=use_deep_layers)

    def act(self, inputs, deterministic=False, u=None):
        """-> value (n, 1), action (n,) [(n, 1) when deterministic, as in the reference], log-probabilities (n, 1).
        u (n,) in [0, 1): draw by inverting the cumulative distribution at u, the rule of csrc/ppo_policy.h, instead of
        Categorical.sample() -- the same uniforms then give the same actions as the one-launch collection."""
        value, dist = self.head(self.base(inputs))
        if deterministic:
            action = dist.probs.argmax(dim=-1, keepdim=True)
        elif u is not None:
            d = (dist.logits - dist.logits.max(dim=-1, keepdim=True).values).double()
            c = torch.cumsum(torch.exp(d), dim=-1)
            below = c <= u.reshape(-1, 1).double() * c[:, -1:]          # (c ascends: the count is the first index above)
            action = below.sum(dim=-1).clamp(max=c.shape[1] - 1)
        else:
            action = dist.sample()
        log_probs = dist.log_prob(action.squeeze(-1)).view(action.size(0), -1).sum(-1).unsqueeze(-1)
        return value, action, log_probs

    def forward(self, inputs):
        raise NotImplementedError

    def get_value(self, inputs):
        value, _ = self.head(self.base(inputs))
        return value

    def evaluate_actions(self, inputs, action):
        """-> value (n, 1), log-probabilities of `action` (n, 1), mean entropy"""
        value, dist = self.head(self.base(inputs))
        log_probs = dist.log_prob(action.squeeze(-1)).view(action.size(0), -1).sum(-1).unsqueeze(-1)
        return value, log_probs, dist.entropy().mean()

    # ------------------------------------------------------------------------------------------------ the kernel's view
    def kernel_shape(self):
        """(N, H, deep) when stove_ppo_collect serves this policy -- a control base on 4 N inputs, N in 1 .. 6, width 128 -> 32, a head
        of width 1 .. 128 and nine actions --, else None"""
        b, h = self.base, self.head
        if not isinstance(b, SimpleControlBase) or not isinstance(h, DiscreteActionHead):
            return None
        n_in, H = b.main[0].in_features, h.main.out_features
        if n_in % 4 or not 1 <= n_in // 4 <= 6 or b.main[0].out_features != 128 or b.main[2].out_features != 32 or h.main.in_features != 32:
            return None
        if not 1 <= H <= 128 or h.actor_head.out_features != 9:
            return None
        return n_in // 4, H, bool(h.use_deep_layers)

    def image_kernel_shape(self):
        """(F, H, deep) when stove_ppo_collect_images serves this policy -- SimpleCNNBase without use_grid on 3 F channels, F in 1 .. 4,
        a head of width 1 .. 512 on its 1568 features and nine actions --, else None"""
        b, h = self.base, self.head
        if not isinstance(b, SimpleCNNBase) or b.use_grid or not isinstance(h, DiscreteActionHead):
            return None
        c, H = b.main[0].in_channels, h.main.out_features
        if c % 3 or not 1 <= c // 3 <= 4 or h.main.in_features != 32 * 7 * 7 or not 1 <= H <= 512 or h.actor_head.out_features != 9:
            return None
        return c // 3, H, bool(h.use_deep_layers)

    def _image_layers(self):
        if self.image_kernel_shape() is None:
            raise ValueError('the one-launch collection on images serves Policy((32, 32, 3 F), 9) without use_grid, F in 1 .. 4, with a '
                             'head of width 1 .. 512 and nine actions')
        b, h = self.base, self.head
        return [b.main[0], b.main[2], h.main] + ([h.in_between[0], h.in_between[2]] if h.use_deep_layers else [])

    def flat_image_params(self):
        """the float32 image stove_ppo_collect_images reads (include/stove_hip.h, next to stove_ppo_image_param_floats): base.main.0
        (48 F -> 32, k = (c * 4 + ky) * 4 + kx), base.main.2 (288 -> 32, k = (c * 3 + ky) * 3 + kx), head.main (1568 -> H) [, the two
        in_between layers with use_deep_layers], then the two heads side by side -- each as its transposed weight (in, out), row-major,
        followed by its bias (out)."""
        h = self.head
        layers = [(l.weight.reshape(l.weight.shape[0], -1), l.bias) for l in self._image_layers()]
        layers.append((torch.cat([h.values_head.weight, h.actor_head.weight], 0), torch.cat([h.values_head.bias, h.actor_head.bias], 0)))
        with torch.no_grad():
            return torch.cat([p for w, bias in layers for p in (w.t().reshape(-1), bias.reshape(-1))]).float().contiguous()

    def load_flat_image_params(self, image):
        """the inverse of flat_image_params(): the layers' weights and biases written from the image, in place"""
        layers, h = self._image_layers(), self.head
        H = h.main.out_features
        if not isinstance(image, torch.Tensor) or image.dim() != 1 or \
                image.numel() != sum(l.weight.numel() + l.bias.numel() for l in layers) + (H + 1) * 10:
            raise ValueError('load_flat_image_params: the image does not have the length of flat_image_params()')
        at = 0

        def take(count):
            nonlocal at
            at += count
            return image[at - count:at]
        with torch.no_grad():
            for layer in layers:
                out, k = layer.weight.shape[0], layer.weight[0].numel()
                layer.weight.copy_(take(out * k).reshape(k, out).t().reshape(layer.weight.shape))
                layer.bias.copy_(take(out))
            heads = take(H * 10).reshape(H, 10).t()
            h.values_head.weight.copy_(heads[:1])
            h.actor_head.weight.copy_(heads[1:])
            bias = take(10)
            h.values_head.bias.copy_(bias[:1])
            h.actor_head.bias.copy_(bias[1:])

    def flat_params(self):
        """the float32 image stove_ppo_collect reads (include/stove_hip.h, next to stove_ppo_param_floats): the layers in order -- base.main.0,
        base.main.2, head.main [, head.in_between.0, head.in_between.2 with use_deep_layers], then the two heads side by side (column 0 the
        value head, columns 1 .. 9 the actor head) --, each as its transposed weight (in, out), row-major, followed by its bias (out)."""
        if self.kernel_shape() is None:
            raise ValueError('flat_params: the one-launch collection serves Policy(base="control") on 4 N inputs (N in 1 .. 6) with a '
                             'head of width 1 .. 128 and nine actions')
        b, h = self.base, self.head
        layers = [(b.main[0].weight, b.main[0].bias), (b.main[2].weight, b.main[2].bias), (h.main.weight, h.main.bias)]
        if h.use_deep_layers:
            layers += [(h.in_between[0].weight, h.in_between[0].bias), (h.in_between[2].weight, h.in_between[2].bias)]
        layers.append((torch.cat([h.values_head.weight, h.actor_head.weight], 0), torch.cat([h.values_head.bias, h.actor_head.bias], 0)))
        with torch.no_grad():
            return torch.cat([p for w, bias in layers for p in (w.t().reshape(-1), bias.reshape(-1))]).float().contiguous()

    def load_flat_params(self, image):
        """the inverse of flat_params(): the layers' weights and biases written from the image, in place"""
        if self.kernel_shape() is None:
            raise ValueError('load_flat_params: the image is that of Policy(base="control") on 4 N inputs (N in 1 .. 6) with a head of '
                             'width 1 .. 128 and nine actions')
        b, h = self.base, self.head
        layers = [b.main[0], b.main[2], h.main] + ([h.in_between[0], h.in_between[2]] if h.use_deep_layers else [])
        H = h.main.out_features
        if not isinstance(image, torch.Tensor) or image.dim() != 1 or \
                image.numel() != sum(l.weight.numel() + l.bias.numel() for l in layers) + (H + 1) * 10:
            raise ValueError('load_flat_params: the image does not have the length of flat_params()')
        at = 0

        def take(count):
            nonlocal at
            at += count
            return image[at - count:at]
        with torch.no_grad():
            for layer in layers:
                out, k = layer.weight.shape
                layer.weight.copy_(take(out * k).reshape(k, out).t())
                layer.bias.copy_(take(out))
            heads = take(H * 10).reshape(H, 10).t()
            h.values_head.weight.copy_(heads[:1])
            h.actor_head.weight.copy_(heads[1:])
            bias = take(10)
            h.values_head.bias.copy_(bias[:1])
            h.actor_head.bias.copy_(bias[1:])
