"""What ``UNet2DModel`` (and ``NCSNppModel`` through it) and ``VQModel`` share below their launch sequences: every parameter is a view of ONE flat
fp32 buffer, registered under the diffusers dotted name, and the layer helpers ``_Conv`` / ``_Norm`` / ``_Attn`` (unet.py) talk to their network
through a handful of names.

* Layers declare their parameters while the network is constructed (``_decl`` / ``_decl_qkv``); ``_materialise`` then lays them out as
  ``[a head the subclass supplies][per attention: q, k, v weights, then biases][everything declared, in order]``, every offset a multiple of 4 floats,
  allocates ``flat_param`` -- and ``flat_grad`` for a network that trains -- and builds the ``P`` / ``Pq`` (``G`` / ``Gq``) views.
* ``input_gradients()`` is the one switch for "differentiate with respect to the input as well".
* A network without gradients answers what ``_Conv.bwd`` / ``_Norm.bwd`` / ``_Attn.bwd`` ask of it with nothing: only the input-gradient halves
  run, on the current stream.  A network that trains (``UNet2DModel``) overrides these with its queues and pools.
"""
from __future__ import annotations

import contextlib
import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops

LEGACY_ATTN = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}     # diffusers < 0.17 names


class _Node(nn.Module):
    """Anonymous container used to reproduce diffusers' dotted state-dict names."""


def _ensure_path(root: nn.Module, parts: Sequence[str]) -> nn.Module:
    m = root
    for p in parts:
        if p not in m._modules:
            m.add_module(p, _Node())
        m = m._modules[p]
    return m


class _NoGrads:
    """What a network without gradients hands `_Conv.bwd` / `_Attn.bwd` where they name a gradient view: nothing is ever written through it."""

    def __getitem__(self, key):
        return self

    def view(self, *shape):
        return self


class FlatParamNet(nn.Module):
    """The flat parameter store, the input-gradient switch and a frozen network's answers to the layer helpers."""

    # ------------------------------------------------------------------------------------------ declarations
    def _begin_declarations(self, device=None):
        """The device (`device`, else the current GPU, else "cpu": structure-only use -- state-dict surgery, tests; any compute call still fails loudly
        in lib.require_device()) and the empty declaration lists; the layers' constructors fill them in the order of the flat buffer."""
        if device is not None:
            self._dev = torch.device(device)
        elif torch.cuda.is_available():
            self._dev = torch.device("cuda", torch.cuda.current_device())
        else:
            self._dev = torch.device("cpu")
        self._decls: List[Tuple[str, Tuple[int, ...], dict]] = []
        self._qkv: List[Tuple[str, int]] = []

    def _decl(self, name, shape, fan_in=None, is_bias=False, ones=False, zeros=False, codebook=False, fourier=False):
        """How reset_parameters fills it: ones / zeros, else U(+-bound) from fan_in (codebook: from the number of entries); fourier marks NCSN++'s fixed
        random features, which NCSNppModel.reset_parameters then overwrites."""
        self._decls.append((name, tuple(shape), dict(fan_in=fan_in, is_bias=is_bias, ones=ones, zeros=zeros, codebook=codebook, fourier=fourier)))

    def _decl_qkv(self, prefix, ch):
        self._qkv.append((prefix, ch))
        return prefix + "::qkv_w", prefix + "::qkv_b"

    # ------------------------------------------------------------------------------------------ layout
    def _materialise(self, head=(), grads=False):
        """head: (name, shape, init) rows laid out first.  grads: a flat gradient buffer too, with the parameters' .grad as views of it."""
        layout = list(head)
        for prefix, ch in self._qkv:                 # q, k, v adjacent: one [3C, C] projection per attention block
            for n in ("to_q", "to_k", "to_v"):
                layout.append((f"{prefix}.{n}.weight", (ch, ch), dict(fan_in=ch)))
            for n in ("to_q", "to_k", "to_v"):
                layout.append((f"{prefix}.{n}.bias", (ch,), dict(fan_in=ch, is_bias=True)))
        layout.extend(self._decls)
        offs, total = {}, 0
        for name, shape, _ in layout:
            n = int(math.prod(shape))
            offs[name] = (total, n, shape)
            total += (n + 3) // 4 * 4               # keep every parameter 16-byte aligned
        self._layout, self._offs, self.flat_numel = layout, offs, total
        self.flat_param = torch.zeros(total, device=self._dev, dtype=torch.float32)
        self.P: Dict[str, torch.Tensor] = {}
        self.Pq: Dict[str, torch.Tensor] = {}
        stores = [(self.flat_param, self.P, self.Pq)]
        if grads:
            self.flat_grad = torch.zeros(total, device=self._dev, dtype=torch.float32)
            self.G: Dict[str, torch.Tensor] = {}
            self.Gq: Dict[str, torch.Tensor] = {}
            stores.append((self.flat_grad, self.G, self.Gq))
        for name, shape, _ in layout:
            off, n, _ = offs[name]
            parts = name.split(".")
            p = nn.Parameter(self.flat_param[off:off + n].view(shape), requires_grad=grads)
            self.P[name] = p.data
            if grads:
                p.grad = self.G[name] = self.flat_grad[off:off + n].view(shape)
            _ensure_path(self, parts[:-1]).register_parameter(parts[-1], p)
        for prefix, ch in self._qkv:
            ow, ob = offs[f"{prefix}.to_q.weight"][0], offs[f"{prefix}.to_q.bias"][0]
            for flat, _, fused in stores:
                fused[prefix + "::qkv_w"] = flat[ow:ow + 3 * ch * ch].view(3 * ch, ch)
                fused[prefix + "::qkv_b"] = flat[ob:ob + 3 * ch]
        self.reset_parameters()

    def _init_bound(self, shape, init) -> float:
        """U(-bound, bound): torch's default init of Conv2d / Linear (kaiming_uniform(a=sqrt(5)) = 1/sqrt(fan_in)); a codebook 1/n_e like upstream
        VectorQuantizer."""
        return 1.0 / shape[0] if init.get("codebook") else 1.0 / math.sqrt(init["fan_in"])

    @torch.no_grad()
    def reset_parameters(self, seed: Optional[int] = None):
        """torch default init of Conv2d / Linear / GroupNorm, drawn on the host in layout order."""
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        host = torch.zeros(self.flat_numel, dtype=torch.float32)
        for name, shape, init in self._layout:
            off, n, _ = self._offs[name]
            if init.get("ones"):
                host[off:off + n] = 1.0
            elif init.get("zeros"):
                host[off:off + n] = 0.0
            else:
                host[off:off + n] = (torch.rand(n, generator=gen) * 2 - 1) * self._init_bound(shape, init)
        self.flat_param.copy_(host)

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = {}
        for k, v in state_dict.items():
            parts = k.split(".")
            if "attentions" in parts and len(parts) >= 2 and parts[-2] in LEGACY_ATTN:
                parts[-2] = LEGACY_ATTN[parts[-2]]
                k = ".".join(parts)
            sd[k] = v
        missing = [k for k in self._offs if k not in sd]
        unexpected = [k for k in sd if k not in self._offs]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:5]}..., unexpected {unexpected[:5]}...")
        with torch.no_grad():
            for k, v in sd.items():
                if k in self._offs:
                    off, n, shape = self._offs[k]
                    assert v.numel() == n, (k, v.shape, shape)
                    self.flat_param[off:off + n].copy_(v.reshape(-1).to(torch.float32))
        self.weights_changed()
        return SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)

    def weights_changed(self):
        """Hook for operands derived from the weights (UNet2DModel's packed split-precision operands); a network without any has nothing to drop."""

    def to(self, *args, **kwargs):          # parameters are views of one flat device buffer: never re-materialise
        return self

    def cuda(self, device=None):
        return self

    @property
    def device(self):
        return self._dev

    @property
    def dtype(self):
        return torch.float32

    # ------------------------------------------------------------------------------------------ the input-gradient switch
    _input_grad = False                     # class default; UNet2DModel: True

    @contextlib.contextmanager
    def input_gradients(self):
        """While open, THIS instance differentiates with respect to its input too: `UNet2DModel.forward` / `NCSNppModel.forward` give a sample that
        requires grad its gradient from the backward pass (with every parameter frozen that pass is the input-gradient pass, `_run_backward`,
        weights=False), and `VQModel.encode(x)` of an x that requires grad keeps a tape and returns latents with a grad_fn.  Forward AND backward
        belong inside.  It nests; the previous state comes back on exit, also after an exception; the class attribute is never written and nothing
        stays in the instance's `__dict__`.  Where the class default is already True (`UNet2DModel`) it changes nothing."""
        had = "_input_grad" in self.__dict__
        old = self.__dict__.get("_input_grad")
        self._input_grad = True
        try:
            yield self
        finally:
            if had:
                self._input_grad = old
            else:
                self.__dict__.pop("_input_grad", None)

    # ------------------------------------------------------------------------------------------ a network without gradients
    # What _Conv.bwd / _Norm.bwd / _Attn.bwd ask of their network, answered for one whose weights never get a gradient: no weight gradient, no bias or
    # GroupNorm-parameter sums, no pack pass, no side stream -- the input-gradient halves on the current stream are all that runs.
    _dx_only = True
    G = Gq = _NoGrads()

    def wants_wgrad(self, dw2d) -> bool:
        return False

    def wgrad(self, *args, **kwargs):
        return None

    def rowsum(self, *args, **kwargs):
        return None

    def colsum_later(self, *args, **kwargs):
        return None

    def pack_later(self, t):
        return None

    def scratch_bc(self, B, Cc, slot=0):
        """[B * Cc] floats the GroupNorm backward kernel writes its per-image parameter partials into (never reduced here)."""
        return torch.empty(B * Cc, device=self._dev, dtype=torch.float32)

    def wt_view(self, prefix, M, Cc, T, fresh=True):
        """Transposed weights [C, M*T] of `prefix` for the stride-1 input gradient; transposed once per state of the weights."""
        cache = self.__dict__.setdefault("_wt_cache", {})
        key = (self.flat_param._version, ops.WEIGHTS_EPOCH)
        ent = cache.get(prefix)
        if ent is None or ent[0] != key:
            wt = ent[1] if ent is not None else torch.empty(M * Cc * T, device=self._dev, dtype=torch.float32)
            ops.weight_transpose(self.P[prefix + ".weight"], wt, M, Cc, T)
            ent = cache[prefix] = (key, wt)
        return ent[1].view(Cc, M * T)
