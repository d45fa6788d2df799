"""The vector-Jacobian product of the denoiser with respect to its input image, g = J^T v with J = dD(x; sigma) / dx.

``input_vjp`` runs one eval-mode forward on the bf16 path and a DGRAD-ONLY backward: the data-gradient kernels of the
training backward, down to conv_in's dgrad into the image (csrc/conv_in_dgrad.hip), and none of its weight side -- no
weight-gradient launch, no skip-gate weight reduction, no gain / modulation finish, no embedding-weight GEMM.  It touches no
parameter's ``.grad``, no optimizer arena, no reducer hook and no counter (``networks.rng.step``, ``FORWARD_EPOCH``), and
leaves nothing queued behind.  The mode is the module-level flag ``networks._DGRAD_ONLY``, set for the duration of the
forward and of the backward only.

``open_input_vjp`` is the two-phase form the DPS solvers use: the cotangent of a step depends on D.
"""
from __future__ import annotations

import torch

from . import networks

__all__ = ["input_vjp", "open_input_vjp"]


def _bf16_only(den) -> None:
    if getattr(den, "eval_dtype", "bf16") != "bf16":
        raise ValueError(f"input_vjp: the denoiser evaluates in {den.eval_dtype!r}, a forward-only path; the backward exists "
                         "on the bf16 path: call set_eval_dtype(\"bf16\") (generate: --network_dtype bf16)")


def _check_inputs(x, sigma) -> None:
    if not isinstance(x, torch.Tensor) or not x.dtype.is_floating_point or x.dim() != 4:
        raise ValueError("input_vjp: x must be a floating-point [B, C, H, W] tensor")
    if not x.is_cuda:
        raise ValueError(f"input_vjp: x is on {x.device}; the library's networks run on the GPU only")
    if not isinstance(sigma, torch.Tensor) or sigma.device != x.device:
        raise ValueError(f"input_vjp: sigma must be a tensor on {x.device}")


def _library_parts(model):
    """(owner module, denoiser, embedding module or None) when `model` is this library's EDM / Denoiser (or a bound method
    of one), else None"""
    from .edm import EDM
    owner = getattr(model, "__self__", model)
    if isinstance(owner, EDM):
        return owner, owner.denoiser, owner.embedding
    if isinstance(owner, networks.Denoiser):
        return owner, owner, None
    return None


def open_input_vjp(model, x, sigma, labels_or_embedding=None):
    """-> (D, pullback): D = model(x, sigma, ...) as detached fp32, and ``pullback(cotangent) -> gx``, the fp32 VJP
    J^T cotangent (cotangent: D's shape).  The pullback may be called once; not calling it is fine."""
    parts = _library_parts(model)
    if parts is None:
        # not one of ours (an analytic denoiser, a wrapped net): plain autograd on its forward
        if not isinstance(x, torch.Tensor) or not x.dtype.is_floating_point:
            raise ValueError("input_vjp: x must be a floating-point tensor")
        with torch.enable_grad():
            xr = x.detach().float().requires_grad_()
            D = model(xr, sigma, labels_or_embedding)

        def pullback_generic(cotangent):
            _check_cotangent(cotangent, D)
            (g,) = torch.autograd.grad(D, xr, cotangent.to(D.dtype))
            return g.float()
        return D.detach().float(), pullback_generic

    owner, den, embedding = parts
    _bf16_only(den)
    _check_inputs(x, sigma)
    was_training = owner.training
    owner.eval()
    dev = x.device.index
    try:
        with torch.no_grad():
            if embedding is not None:
                labels = labels_or_embedding if owner.conditional else None
                _, emb = embedding(sigma, labels)
            else:
                if not isinstance(labels_or_embedding, torch.Tensor):
                    raise ValueError("input_vjp: a Denoiser takes the embedding tensor as its fourth argument")
                emb = labels_or_embedding
            emb = emb.detach()
        prev, networks._DGRAD_ONLY[0] = networks._DGRAD_ONLY[0], True
        try:
            with torch.enable_grad():
                xr = x.detach().float().contiguous().requires_grad_()
                D = den(xr, sigma.detach(), emb)
        finally:
            networks._DGRAD_ONLY[0] = prev
    finally:
        owner.train(was_training)

    def pullback(cotangent):
        _check_cotangent(cotangent, D)
        prev, networks._DGRAD_ONLY[0] = networks._DGRAD_ONLY[0], True
        try:
            (g,) = torch.autograd.grad(D, xr, cotangent.detach().float().contiguous())
        finally:
            networks._DGRAD_ONLY[0] = prev
            networks._tail_slot.pop(dev, None)      # (taken by the last block's backward; emptied whatever happened)
        return g
    return D.detach(), pullback


def _check_cotangent(cotangent, D) -> None:
    if not isinstance(cotangent, torch.Tensor) or not cotangent.dtype.is_floating_point:
        raise ValueError("input_vjp: cotangent must be a floating-point tensor")
    if tuple(cotangent.shape) != tuple(D.shape):
        raise ValueError(f"input_vjp: cotangent must have D's shape {tuple(D.shape)}, got {tuple(cotangent.shape)}")
    if cotangent.device != D.device:
        raise ValueError(f"input_vjp: cotangent is on {cotangent.device}, D on {D.device}")


def input_vjp(model, x, sigma, labels_or_embedding=None, cotangent=None):
    """(D, gx): D = model(x, sigma, labels) and gx = J^T cotangent, J = dD / dx, both fp32 [B, C, H, W].

    ``model``: an ``EDM`` (fourth argument: class labels or None) or a ``Denoiser`` (fourth argument: the embedding tensor).
    It is evaluated in eval mode on the bf16 path, and only data gradients are computed (see the module docstring); D equals
    the ``torch.no_grad()`` evaluation bit for bit.  A denoiser whose eval dtype is "f32" / "f32x3" raises ValueError: that
    path is forward-only.  Any other callable ``model(x, sigma, labels)`` goes through ``torch.autograd.grad`` on its forward.
    ``cotangent``: fp32 [B, C, H, W]."""
    if cotangent is None:
        raise ValueError("input_vjp: cotangent is required (the vector of the vector-Jacobian product)")
    D, pullback = open_input_vjp(model, x, sigma, labels_or_embedding)
    return D, pullback(cotangent)
