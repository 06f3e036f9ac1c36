"""CPU restatement of villandiffusion_amd.lora for the tests (a helper module, not a test file; no GPU needed).

The closed forms of the two kernels in float64 with their derived error bounds, and a functional LoRA wrapper of the oracles
(`oracle.unet_ref.UNet2DModelRef`, `oracle.ncsnpp_ref.NCSNppRef`): `torch.func.functional_call` with W0 + s * (B @ A) in place of every adapted
weight, so that autograd gives dA and dB -- nothing here uses the identities dL/dB = s G A^T, dL/dA = s B^T G the HIP path rests on -- and torch
`Adam` on (A, B) only.

Adapters are dicts weight name -> (A [r, L], B [M, r]); `slices` (weight name -> (slice of A, slice of B) in the flat adapter buffer) comes from
`lora.adapter_table`, and `selected` restates the selection rule on the oracle's own parameters so that the table can be checked against it."""
import re

import torch
from torch.func import functional_call

from oracle import schedulers_ref as R
from oracle.loss_ref import SDE_VP, LossFnRef

U = 2.0 ** -24          # unit round-off of f32
_ATTN = re.compile(r"(^|\.)attentions\.\d+\.(to_q|to_k|to_v|to_out\.0)\.weight$")


# ------------------------------------------------------------------------------------------------------------------------------- the selection
def selected(ref, target, r):
    """(adapted, skipped) weight names by the rule of the issue, from the oracle's parameters (order: the oracle's, not the table's)."""
    adapted, skipped = [], []
    for name, p in ref.named_parameters():
        if target == "attn":
            ok = p.dim() >= 2 and _ATTN.search(name) is not None
        elif target == "conv":
            ok = p.dim() == 4 and name.endswith(".weight")
        else:
            ok = p.dim() >= 2
        if ok:
            M = p.shape[0]
            (skipped if min(M, p.numel() // M) <= r else adapted).append(name)
    return adapted, skipped


# ------------------------------------------------------------------------------------------------------------------------------- closed forms
def merged(w0, A, B, s):
    """W0 + s * B A in float64 (w0: [M, L])."""
    return w0.double() + s * (B.double() @ A.double())


def merge_bound(w0, A, B, s):
    """2 (r + 2) u (|w0| + |s| sum_q |B||A|): r products, r additions of the chain, the product with s and the final addition, with a factor 2
    to spare; holds for any order of the sum over q."""
    r = A.shape[0]
    return 2 * (r + 2) * U * (w0.double().abs() + abs(s) * (B.double().abs() @ A.double().abs()))


def grads(G, A, B, s):
    """(dA, dB) = (s B^T G, s G A^T) in float64 (G: the weight gradient, [M, L])."""
    G, A, B = G.double(), A.double(), B.double()
    return s * (B.t() @ G), s * (G @ A.t())


def grad_bounds(G, A, B, s):
    """(bound of dA, bound of dB): 2 (n + 2) u |s| sum |terms| with n the number of addends of that sum (M for dA, L for dB): n products,
    n - 1 additions, the product with s, a factor 2 to spare; holds for any summation order."""
    G, A, B = G.double().abs(), A.double().abs(), B.double().abs()
    M, L = G.shape
    return 2 * (M + 2) * U * abs(s) * (B.t() @ G), 2 * (L + 2) * U * abs(s) * (G @ A.t())


# ------------------------------------------------------------------------------------------------------------------------------- the wrapper
def init_adapters(ref, names, r, seed):
    """The documented initialisation, in the given (table) order: A ~ U(+-1/sqrt(L)) from a CPU Generator(seed), one draw of r * L per layer;
    B = 0.  -> name -> (A, B), f32."""
    gen = torch.Generator().manual_seed(seed)
    params = dict(ref.named_parameters())
    out = {}
    for name in names:
        M = params[name].shape[0]
        L = params[name].numel() // M
        A = ((torch.rand(r * L, generator=gen) * 2 - 1) * (1.0 / L ** 0.5)).view(r, L)
        out[name] = (A, torch.zeros(M, r))
    return out


def flat_of(adapters, slices, numel):
    """The flat adapter buffer (padding zero) of name -> (A, B)."""
    flat = torch.zeros(numel, dtype=next(iter(adapters.values()))[0].dtype)
    for name, (a, b) in slices.items():
        flat[a] = adapters[name][0].detach().reshape(-1)
        flat[b] = adapters[name][1].detach().reshape(-1)
    return flat


def adapters_of(flat, slices, shapes, r):
    """name -> (A [r, L], B [M, r]) views of a flat adapter buffer."""
    out = {}
    for name, (a, b) in slices.items():
        M = shapes[name][0]
        out[name] = (flat[a].view(r, -1), flat[b].view(M, r))
    return out


def adapted_parameters(ref, adapters, s):
    """name -> W0 + s * (B @ A) for functional_call, in the dtype of `ref`."""
    params = dict(ref.named_parameters())
    return {name: params[name].detach() + s * (B.to(params[name].dtype) @ A.to(params[name].dtype)).view_as(params[name])
            for name, (A, B) in adapters.items()}


def call(ref, adapters, s, x, t):
    """The adapted oracle's output (sample) at (x, t)."""
    out = functional_call(ref, adapted_parameters(ref, adapters, s), (x, t))
    return out[0] if isinstance(out, (tuple, list)) else getattr(out, "sample", out)


def autograd_grads(ref, adapters, s, x, t, w):
    """dA, dB of sum(model(x, t) * w) by autograd through W0 + s * B @ A: name -> (dA, dB); and the ordinary weight gradients dW of the same
    loss at the merged weights: name -> dW [M, L]."""
    dtype = next(ref.parameters()).dtype
    leaves = {n: (A.detach().to(dtype).requires_grad_(True), B.detach().to(dtype).requires_grad_(True)) for n, (A, B) in adapters.items()}
    merged_w = adapted_parameters(ref, leaves, s)
    for v in merged_w.values():
        v.retain_grad()
    out = functional_call(ref, merged_w, (x.to(dtype), t))
    y = out[0] if isinstance(out, (tuple, list)) else getattr(out, "sample", out)
    (y * w.to(dtype)).sum().backward()
    gab = {n: (a.grad.detach(), b.grad.detach()) for n, (a, b) in leaves.items()}
    gw = {n: v.grad.detach().reshape(v.shape[0], -1) for n, v in merged_w.items()}
    return gab, gw, y.detach()


class AdamOnAdapters:
    """The trainer's LoRA step on the oracle: the VP loss of the adapted network, clip_grad_norm_(A's and B's, 1.0), torch Adam on them with
    the cosine-with-warm-up schedule -- what `Trainer(lora=...)` is held to."""

    def __init__(self, ref, adapters, s, lr, total_steps, warmup_steps=0, max_grad_norm=1.0):
        self.ref, self.s, self.max_grad_norm = ref, s, max_grad_norm
        for p in ref.parameters():
            p.requires_grad_(False)
        self.adapters = {n: (A.detach().clone().requires_grad_(True), B.detach().clone().requires_grad_(True)) for n, (A, B) in adapters.items()}
        self.leaves = [p for ab in self.adapters.values() for p in ab]
        self.opt = torch.optim.Adam(self.leaves, lr=lr)
        self.sch = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda k: R.cosine_with_warmup_lambda(k, warmup_steps, total_steps))
        self.lf = LossFnRef(R.DDPMSchedulerRef(), SDE_VP, psi=1)

    def step(self, x0, Rr, t, eps):
        model = lambda x, tt, return_dict=False: functional_call(self.ref, adapted_parameters(self.ref, self.adapters, self.s), (x, tt))
        loss = self.lf.p_loss(model, x0, Rr, t, noise=eps)
        value = float(loss.detach())
        loss.backward()
        if self.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.leaves, self.max_grad_norm)
        self.opt.step()
        self.sch.step()
        self.opt.zero_grad()
        return value

    def merged_state(self):
        """name -> merged weight, every parameter of the oracle (the frozen ones as they are)."""
        sd = {k: v.detach().clone() for k, v in self.ref.state_dict().items()}
        for name, w in adapted_parameters(self.ref, self.adapters, self.s).items():
            sd[name] = w.detach()
        return sd
