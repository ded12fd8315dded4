"""Activation table of the SI models (reference: subgraph_isomorphism/utils/act.py:457-489).

The reference returns SHARED singleton modules from a global dict; stateless activations make that
unobservable, so fresh modules are created here (PReLU would otherwise share one parameter across layers --
SURVEY.md appendix A)."""
import torch as th
import torch.nn as nn

LEAKY_RELU_A = 1 / 5.5  # reference: constants.py:10


class Identity(nn.Module):
    def forward(self, x):
        return x


class Sparsemax(nn.Module):
    """Sparsemax along `dim` (act.py:255-316; Martins & Astudillo 2016): the Euclidean projection of the scores onto the simplex.
    With z sorted descending, k = max{j : 1 + j z_(j) > sum_{i <= j} z_(i)} and tau = (sum_{i <= k} z_(i) - 1) / k; the output is
    max(z - tau, 0).  The scores are shifted by their maximum first, as the reference does (a key at -1e30 never enters the support)."""

    def __init__(self, dim=-1):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        dim = self.dim
        x = x - th.max(x, dim=dim, keepdim=True)[0]
        zs = th.sort(x, dim=dim, descending=True)[0]
        shape = [1] * x.dim()
        shape[dim] = -1
        rg = th.arange(1, x.size(dim) + 1, device=x.device, dtype=x.dtype).view(shape)
        is_gt = th.gt(1 + rg * zs, th.cumsum(zs, dim)).to(x.dtype)
        k = th.max(is_gt * rg, dim, keepdim=True)[0]
        taus = (th.sum(is_gt * zs, dim, keepdim=True) - 1) / k
        return th.max(th.zeros_like(x), x - taus)

    def extra_repr(self):
        return "dim={}".format(self.dim)


_FACTORY = {
    "none": Identity,
    "sigmoid": nn.Sigmoid,
    "tanh": nn.Tanh,
    "relu": nn.ReLU,
    "relu6": nn.ReLU6,
    "leaky_relu": lambda: nn.LeakyReLU(negative_slope=LEAKY_RELU_A),
    "prelu": lambda: nn.PReLU(init=LEAKY_RELU_A),
    "elu": nn.ELU,
    "celu": nn.CELU,
    "selu": nn.SELU,
    "gelu": nn.GELU,
    "softmax": lambda: nn.Softmax(dim=-1),
    "sparsemax": lambda: Sparsemax(dim=-1),
}


def map_activation_str_to_layer(act_func, **kw):
    if act_func not in _FACTORY:
        raise NotImplementedError(act_func)
    act = _FACTORY[act_func]()
    for k, v in kw.items():
        if hasattr(act, k):
            try:
                setattr(act, k, v)
            except Exception:
                pass
    return act
