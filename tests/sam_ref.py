"""The sharpness-aware optimiser step restated in torch on the oracle (UNet2DModelRef, LossFnRef, torch.optim.Adam, clip_grad_norm_): what
`Trainer(sam=SAMConfig(...))` is held to, plus the inputs and bounds the SAM tests share.

One step: loss and backward at w (g); e = rho * T^2 g / (||T g|| + 1e-12) with
  "sam":    T = 1
  "asam":   T_i = |w_i| + eta
  "neuron": T_j = sqrt(mean_k w_jk^2) + eta for every weight row j of the selected layers (the names of `anp.neuron_table(model, layers).slices`),
            e = 0 for every other float (biases, norms, unselected layers);
loss and backward at w + e (g'); w restored; clip_grad_norm_(1.0), Adam, cosine schedule on g'.  rho = 0 is the plain step."""
import torch

import oracle.schedulers_ref as R
from oracle.loss_ref import SDE_VP, LossFnRef

SMALL = dict(sample_size=32, block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8,
             down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))     # tests/test_ema_gpu.py's

# the trajectory cases of tests/test_sam_gpu.py: (mode, rho, eta, layers)
CASES = {"sam": ("sam", 0.05, 0.01, "conv"), "asam": ("asam", 0.5, 0.01, "conv"), "neuron": ("neuron", 0.5, 0.01, "conv")}


def g(seed):
    return torch.Generator().manual_seed(seed)


def batch_of(i, B=4):
    """tests/test_ema_gpu.py's batches, on the host."""
    gen = g(100 + i)
    x0 = torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1
    Rr = torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1
    Rr[::2] = 0
    eps = torch.randn(B, 3, 32, 32, generator=gen)
    t = torch.randint(0, 1000, (B,), generator=gen)
    return x0, Rr, t, eps


def perturbation(params, grads, mode, rho, eta=0.01, rows=()):
    """name -> e for every parameter.  params / grads: name -> tensor; rows: the names whose rows are neurons ("neuron" only)."""
    if mode == "sam":
        T2g = {k: grads[k] for k in params}
        nsq = sum((grads[k] ** 2).sum() for k in params)
    elif mode == "asam":
        T = {k: params[k].abs() + eta for k in params}
        T2g = {k: T[k] * T[k] * grads[k] for k in params}
        nsq = sum(((T[k] * grads[k]) ** 2).sum() for k in params)
    elif mode == "neuron":
        T2g, nsq = {k: torch.zeros_like(params[k]) for k in params}, 0.0
        for k in rows:
            w, gr = params[k].reshape(params[k].shape[0], -1), grads[k].reshape(params[k].shape[0], -1)
            T = ((w ** 2).sum(1) / w.shape[1]).sqrt() + eta
            nsq = nsq + (T * T * (gr ** 2).sum(1)).sum()
            T2g[k] = ((T * T)[:, None] * gr).reshape(params[k].shape)
    else:
        raise ValueError(mode)
    c = rho / (torch.as_tensor(nsq).sqrt() + 1e-12)
    return {k: c * T2g[k] for k in params}


class SamOnOracle:
    """mode None: the plain step (one pass).  step() returns (loss at w, loss at w + e or None)."""

    def __init__(self, ref, mode, rho=0.0, eta=0.01, rows=(), lr=1e-3, total_steps=20, warmup_steps=0, max_grad_norm=1.0, lf=None):
        self.ref, self.mode, self.rho, self.eta, self.rows, self.max_grad_norm = ref, mode, rho, eta, tuple(rows), max_grad_norm
        self.named = dict(ref.named_parameters())
        self.opt = torch.optim.Adam(ref.parameters(), lr=lr)
        self.sch = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda k: R.cosine_with_warmup_lambda(k, warmup_steps, total_steps))
        self.lf = lf if lf is not None else LossFnRef(R.DDPMSchedulerRef(), SDE_VP, psi=1)
        self.last_e = None

    def _pass(self, x0, Rr, t, eps):
        self.opt.zero_grad()
        loss = self.lf.p_loss(self.ref, x0, Rr, t, noise=eps)
        loss.backward()
        return float(loss.detach())

    def step(self, x0, Rr, t, eps):
        l1, l2 = self._pass(x0, Rr, t, eps), None
        if self.mode is not None:
            with torch.no_grad():
                params = {k: p.detach() for k, p in self.named.items()}
                e = perturbation(params, {k: p.grad for k, p in self.named.items()}, self.mode, self.rho, self.eta, self.rows)
                backup = {k: p.detach().clone() for k, p in self.named.items()}
                for k, p in self.named.items():
                    p.add_(e[k])
            self.last_e = e
            l2 = self._pass(x0, Rr, t, eps)
            with torch.no_grad():
                for k, p in self.named.items():
                    p.copy_(backup[k])
        if self.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.ref.parameters(), self.max_grad_norm)
        self.opt.step()
        self.sch.step()
        self.opt.zero_grad()
        return l1, l2


def update_l2_error(got, want, start):
    """tests/test_train_sample_gpu.py's trajectory metric: ||theta - theta_ref|| / ||theta_ref - theta_0|| over every parameter (name -> tensor)."""
    num = sum(float(((got[k].detach().cpu().double() - v.detach().double()) ** 2).sum()) for k, v in want.items())
    den = sum(float(((v.detach().double() - start[k].double()) ** 2).sum()) for k, v in want.items())
    return (num / den) ** 0.5


# ---- the kernels' sums: the longest addition chains include/villan_hip.h states, and the bound the tests derive from them ----------------------
def norm_chain(n, grid, block):
    """vd_sam_norm_sq: ceil(ceil(n / 4) / (grid * block)) + ceil(grid / 256) + 18."""
    items = (n + 3) // 4
    return -(-items // (grid * block)) + -(-grid // 256) + 18


def coef_chain(jobs):
    """vd_sam_neuron_coef: sum over the jobs of ceil(rows / 256), plus 8."""
    return sum(-(-j[1] // 256) for j in jobs) + 8


def sum_bound(chain, terms):
    """chain * 2^-24 * sum |terms| (terms: float64)."""
    return chain * 2.0 ** -24 * float(terms.abs().sum())
