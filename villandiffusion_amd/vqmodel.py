"""VQ-VAE (``VQModel``) of the latent-diffusion path on the HIP kernels of the UNet: forward only, and -- inside ``with vq.input_gradients():``
-- the encoder's input gradient (``defense_ldm`` pulls dL/dlatents back to a pixel trigger with it).

Reference use: ``vae.encode(x).latents`` / ``vae.decode(z).sample`` in loss.py:942-962,
VillanDiffusion.py:378,472 and inside the LDM pipeline (model.py:713); the reference freezes it
(``vae.requires_grad_(False)``, model.py:790), so no parameter ever gets a gradient here.  Architecture = diffusers ``VQModel``
(Encoder -> quant_conv -> VectorQuantizer -> post_quant_conv -> Decoder), state-dict names as in diffusers so the
``vqvae/`` folder of ``CompVis/ldm-celebahq-256`` loads unchanged (legacy attention key names are mapped).

Every tensor op is a launch through the C ABI (3x3 convs incl. the fused nearest-2x upsample and the padded stride-2
downsample, GroupNorm+SiLU, 1x1 convs, attention GEMMs + column softmax, ``vd_vq_nearest``); parameters are views of one
flat fp32 buffer like the UNet's.

The encoder's input gradient is a launch sequence over the input-gradient halves of ``_Conv.bwd`` / ``_Norm.bwd`` / ``_Attn.bwd``, the way the
UNet's frozen-weight pass uses them: the network answers their weight-gradient, row-sum, column-sum and pack requests with nothing, on the
current stream (the defaults of ``flatnet.FlatParamNet``, which also holds the flat buffer and the switch).  ``decode`` stays forward-only.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import ops
from .flatnet import FlatParamNet
from .lib import B_CONV3_S2, B_CONV3_UP
from .unet import _Attn, _Conv, _Norm, _conv1x1_dgrad


class _ResnetNoTemb:
    """ResnetBlock2D(temb_channels=None): conv2(silu(gn(conv1(silu(gn(x)))))) + shortcut(x)."""

    def __init__(self, net, prefix, cin, cout):
        self.net, self.prefix, self.cin, self.cout = net, prefix, cin, cout
        self.norm1 = _Norm(net, prefix + ".norm1", cin, True)
        self.conv1 = _Conv(net, prefix + ".conv1", cin, cout)
        self.norm2 = _Norm(net, prefix + ".norm2", cout, True)
        self.conv2 = _Conv(net, prefix + ".conv2", cout, cout)
        self.has_sc = cin != cout
        if self.has_sc:
            net._decl(prefix + ".conv_shortcut.weight", (cout, cin, 1, 1), fan_in=cin)
            net._decl(prefix + ".conv_shortcut.bias", (cout,), fan_in=cin, is_bias=True)

    def fwd(self, x, tape=None):
        net = self.net
        B, _, H, W = x.shape
        a1 = torch.empty_like(x)
        m1, r1 = self.norm1.fwd(x, a1)
        h1 = torch.empty((B, self.cout, H, W), device=x.device, dtype=torch.float32)
        self.conv1.fwd(a1, h1)
        del a1
        a2 = torch.empty_like(h1)
        m2, r2 = self.norm2.fwd(h1, a2)
        if tape is None:
            out = h1                                 # conv2 does not read h1: reuse its storage for the block output
        else:
            out = torch.empty_like(h1)               # (norm2's backward reads h1)
            tape.append(("res", self, (x, m1, r1, h1, m2, r2)))
        if self.has_sc:
            ops.conv1x1(x, net.P[self.prefix + ".conv_shortcut.weight"].view(self.cout, self.cin),
                        net.P[self.prefix + ".conv_shortcut.bias"], out)
            self.conv2.fwd(a2, out, residual=out)
        else:
            self.conv2.fwd(a2, out, residual=x)
        return out

    def bwd(self, saved, dout):
        """dL/dx of the block: the input-gradient halves only (the activations a weight gradient would read were never kept)."""
        x, m1, r1, h1, m2, r2 = saved
        da2 = torch.empty_like(h1)
        self.conv2.bwd(dout, None, da2, skip_bias=True)
        dh1 = torch.empty_like(h1)
        self.norm2.bwd(da2, h1, m2, r2, dh1)
        da1 = da2 if self.cin == self.cout else torch.empty_like(x)
        self.conv1.bwd(dh1, None, da1, skip_bias=True)
        dsc = _conv1x1_dgrad(self.net, self.prefix + ".conv_shortcut", self.cout, self.cin, dout) if self.has_sc else dout
        return self.norm1.bwd(da1, x, m1, r1, torch.empty_like(x), extra=dsc)


class _Mid:
    def __init__(self, net, prefix, ch):
        self.r0 = _ResnetNoTemb(net, prefix + ".resnets.0", ch, ch)
        self.attn = _Attn(net, prefix + ".attentions.0", ch, None)
        self.r1 = _ResnetNoTemb(net, prefix + ".resnets.1", ch, ch)

    def fwd(self, h, tape=None):
        sub = None if tape is None else []
        h = self.r0.fwd(h, sub)
        out = torch.empty_like(h)
        sa = self.attn.fwd(h, out, None, sub is not None)
        out = self.r1.fwd(out, sub)
        if tape is not None:
            tape.append(("mid", self, (sub[0][2], sa, sub[1][2])))
        return out

    def bwd(self, saved, dout):
        s0, sa, s1 = saved
        g = self.r1.bwd(s1, dout)
        g = self.attn.bwd(sa, g, torch.empty_like(g), None)
        return self.r0.bwd(s0, g)


class _VQEncodeFn(torch.autograd.Function):
    """latents = VQModel.encode(x) with a tape; backward is the encoder's input-gradient pass (dL/dx only: the weights are frozen)."""

    @staticmethod
    def forward(ctx, net, x):
        tape = []
        lat = net._encode(x, tape)
        ctx.net, ctx.tape = net, tape
        return lat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlat):
        net, tape = ctx.net, ctx.tape
        ctx.tape = None
        if tape is None:
            raise RuntimeError("VQModel.encode: the tape of this forward pass has been used (one backward per encode)")
        return None, net._encode_backward(tape, dlat.contiguous())


class VQModel(FlatParamNet):
    """Drop-in for diffusers ``VQModel`` on the inference surface the reference uses: ``.encode(x).latents``,
    ``.decode(z).sample``, ``.config``, ``.device``, ``.eval()``, ``.requires_grad_``, ``state_dict``/``load_state_dict``."""

    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",) * 3,
                 up_block_types=("UpDecoderBlock2D",) * 3, block_out_channels=(128, 256, 512), layers_per_block=2, act_fn="silu",
                 latent_channels=3, sample_size=256, num_vq_embeddings=8192, norm_num_groups=32, vq_embed_dim=None,
                 scaling_factor=0.18215, norm_eps=1e-6, device=None, **unused):
        super().__init__()
        if act_fn != "silu" or any(t != "DownEncoderBlock2D" for t in down_block_types) or \
                any(t != "UpDecoderBlock2D" for t in up_block_types):
            raise NotImplementedError("only the published VQModel configuration family (silu, Down/UpDecoderBlock2D) is implemented")
        vq_embed_dim = vq_embed_dim if vq_embed_dim is not None else latent_channels
        boc = tuple(block_out_channels)
        self.config = SimpleNamespace(
            in_channels=in_channels, out_channels=out_channels, down_block_types=tuple(down_block_types),
            up_block_types=tuple(up_block_types), block_out_channels=boc, layers_per_block=layers_per_block, act_fn=act_fn,
            latent_channels=latent_channels, sample_size=sample_size, num_vq_embeddings=num_vq_embeddings,
            norm_num_groups=norm_num_groups, vq_embed_dim=vq_embed_dim, scaling_factor=scaling_factor)
        self.groups, self.eps = norm_num_groups, norm_eps
        self._begin_declarations(device)

        # ---- encoder ----
        self.e_in = _Conv(self, "encoder.conv_in", in_channels, boc[0])
        self.e_blocks, ch = [], boc[0]
        for i, oc in enumerate(boc):
            res = [_ResnetNoTemb(self, f"encoder.down_blocks.{i}.resnets.{j}", ch if j == 0 else oc, oc) for j in range(layers_per_block)]
            ds = _Conv(self, f"encoder.down_blocks.{i}.downsamplers.0.conv", oc, oc, mode=B_CONV3_S2) if i != len(boc) - 1 else None
            self.e_blocks.append((res, ds))
            ch = oc
        self.e_mid = _Mid(self, "encoder.mid_block", ch)
        self.e_norm = _Norm(self, "encoder.conv_norm_out", ch, True)
        self.e_out = _Conv(self, "encoder.conv_out", ch, latent_channels)
        # ---- quantiser ----
        self._decl("quant_conv.weight", (vq_embed_dim, latent_channels, 1, 1), fan_in=latent_channels)
        self._decl("quant_conv.bias", (vq_embed_dim,), fan_in=latent_channels, is_bias=True)
        self._decl("quantize.embedding.weight", (num_vq_embeddings, vq_embed_dim), codebook=True)
        self._decl("post_quant_conv.weight", (latent_channels, vq_embed_dim, 1, 1), fan_in=vq_embed_dim)
        self._decl("post_quant_conv.bias", (latent_channels,), fan_in=vq_embed_dim, is_bias=True)
        # ---- decoder ----
        rev = list(reversed(boc))
        self.d_in = _Conv(self, "decoder.conv_in", latent_channels, rev[0])
        self.d_mid = _Mid(self, "decoder.mid_block", rev[0])
        self.d_blocks, ch = [], rev[0]
        for i, oc in enumerate(rev):
            res = [_ResnetNoTemb(self, f"decoder.up_blocks.{i}.resnets.{j}", ch if j == 0 else oc, oc) for j in range(layers_per_block + 1)]
            us = _Conv(self, f"decoder.up_blocks.{i}.upsamplers.0.conv", oc, oc, mode=B_CONV3_UP) if i != len(rev) - 1 else None
            self.d_blocks.append((res, us))
            ch = oc
        self.d_norm = _Norm(self, "decoder.conv_norm_out", ch, True)
        self.d_out = _Conv(self, "decoder.conv_out", ch, out_channels)
        self._materialise()

    # ------------------------------------------------------------------------------------------ forward launch sequences
    def _conv1x1(self, name, x):
        w = self.P[name + ".weight"]
        out = torch.empty((x.shape[0], w.shape[0], x.shape[2], x.shape[3]), device=x.device, dtype=torch.float32)
        return ops.conv1x1(x, w.view(w.shape[0], w.shape[1]), self.P[name + ".bias"], out)

    @staticmethod
    def _new(x, ch, scale=1.0):
        B, _, H, W = x.shape
        return torch.empty((B, ch, int(H * scale), int(W * scale)), device=x.device, dtype=torch.float32)

    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """latents = quant_conv(Encoder(x)); NOT quantised (upstream VQModel.encode).  Inside `input_gradients()` only, an x that requires grad
        keeps a tape and the latents get a grad_fn: `torch.autograd.grad(lat, x, dlat)` is then the encoder's input-gradient pass.  Whatever the
        parameters' requires_grad flags say, no parameter gradient is computed or written."""
        if self._input_grad and torch.is_grad_enabled() and x.requires_grad:
            lat = _VQEncodeFn.apply(self, x.to(self._dev, torch.float32).contiguous())
        else:
            with torch.no_grad():
                lat = self._encode(x.to(self._dev, torch.float32).contiguous(), None)
        return SimpleNamespace(latents=lat) if return_dict else (lat,)

    def _encode(self, x, tape):
        """The encoder's launch sequence.  tape: None, or the list that receives one record per differentiated layer, in forward order."""
        h = self._new(x, self.e_in.cout)
        self.e_in.fwd(x, h)
        for res, ds in self.e_blocks:
            for r in res:
                h = r.fwd(h, tape)
            if ds is not None:
                o = self._new(h, ds.cout, 0.5)
                ds.fwd(h, o)
                if tape is not None:
                    tape.append(("conv", ds, h.shape))
                h = o
        h = self.e_mid.fwd(h, tape)
        a = torch.empty_like(h)
        m, r = self.e_norm.fwd(h, a)
        z = self._new(a, self.e_out.cout)
        self.e_out.fwd(a, z)
        if tape is not None:
            tape.append(("norm", self.e_norm, (h, m, r)))
            tape.append(("conv", self.e_out, a.shape))
        return self._conv1x1("quant_conv", z)

    def _encode_backward(self, tape, dlat):
        """dL/dx from dL/dlatents: quant_conv's input gradient, the tape backwards, conv_in's input gradient."""
        vq_dim, lat_ch = self.P["quant_conv.weight"].shape[:2]
        g = _conv1x1_dgrad(self, "quant_conv", vq_dim, lat_ch, dlat)
        while tape:
            kind, layer, saved = tape.pop()
            if kind == "conv":                       # conv_out and the padded stride-2 downsamplers: saved is the input's shape
                g = layer.bwd(g, None, torch.empty(saved, device=g.device, dtype=torch.float32), skip_bias=True)
            elif kind == "norm":
                h, m, r = saved
                g = layer.bwd(g, h, m, r, torch.empty_like(h))
            elif kind in ("res", "mid"):
                g = layer.bwd(saved, g)
            else:
                raise RuntimeError(kind)
        B, _, H, W = g.shape
        return self.e_in.bwd(g, None, torch.empty((B, self.e_in.cin, H, W), device=g.device, dtype=torch.float32), skip_bias=True)

    @torch.no_grad()
    def quantize_latents(self, h: torch.Tensor, return_indices: bool = False):
        h = h.to(self._dev, torch.float32).contiguous()
        zq = torch.empty_like(h)
        idx = torch.empty(h.shape[0] * h.shape[2] * h.shape[3], device=h.device, dtype=torch.int64) if return_indices else None
        ops.vq_nearest(h, self.P["quantize.embedding.weight"], zq, idx)
        return (zq, idx) if return_indices else zq

    @torch.no_grad()
    def decode(self, h: torch.Tensor, force_not_quantize: bool = False, return_dict: bool = True):
        """sample = Decoder(post_quant_conv(quantize(h)))  (upstream VQModel.decode)."""
        h = h.to(self._dev, torch.float32).contiguous()
        q = h if force_not_quantize else self.quantize_latents(h)
        q = self._conv1x1("post_quant_conv", q)
        x = self._new(q, self.d_in.cout)
        self.d_in.fwd(q, x)
        x = self.d_mid.fwd(x)
        for res, us in self.d_blocks:
            for r in res:
                x = r.fwd(x)
            if us is not None:
                o = self._new(x, us.cout, 2.0)
                us.fwd(x, o)
                x = o
        a = torch.empty_like(x)
        self.d_norm.fwd(x, a)
        out = self._new(a, self.d_out.cout)
        self.d_out.fwd(a, out)
        return SimpleNamespace(sample=out) if return_dict else (out,)

    def forward(self, x, return_dict: bool = True):
        return self.decode(self.encode(x).latents, return_dict=return_dict)
