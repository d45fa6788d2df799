"""Tensor-level wrappers around the C-ABI kernels: validate shapes/dtypes on the host (a kernel
that faults can take the whole GPU node down), then pass raw pointers + the current stream.

Layout conventions: activations are NHWC bf16 tensors of shape (B, H, W, C) (contiguous);
"rows" means B*H*W.  Per-(sample,channel) quantities are fp32 (B, C).
"""
import contextlib
import ctypes
import functools
import math
import os
import types
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

bf16, f32 = torch.bfloat16, torch.float32

# When set to a dict, the MFMA kernels below record (start_event, end_event, algorithmic FLOPs, algorithmic
# HBM bytes) per launch on the launch stream (bench.py's roofline leg).  None = no instrumentation.
PROFILE = None


class _prof:
    def __init__(self, name, flops, nbytes):
        self.name, self.flops, self.nbytes = name, flops, nbytes

    def __enter__(self):
        if PROFILE is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if PROFILE is not None:
            self.e.record()
            PROFILE.setdefault(self.name, []).append((self.s, self.e, self.flops, self.nbytes))
        return False


def _stream():
    s = torch.cuda.current_stream()
    if s.device_index not in _lib._inited_devices:
        _lib.init_device(s.device_index)
    return ctypes.c_void_p(s.cuda_stream)


_SIDE_STREAMS = {}


def side_stream(device):
    """Per-device auxiliary HIP stream: weight-gradient kernels (off the backward's critical path) run here, under
    the HBM-bound elementwise kernels of the main stream.  Created on first use."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    s = _SIDE_STREAMS.get(idx)
    if s is None:
        s = _SIDE_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return s


def side_streams():
    return list(_SIDE_STREAMS.values())


class _ZeroPool:
    """Zero-initialised fp32 scratch for the atomically-accumulated outputs (reductions, small weight grads).

    One training step needs ~110 such tensors; a `torch.zeros` each is a fill launch each.  The pool zeroes a
    16 MiB chunk with ONE fill and hands out disjoint 256-byte-aligned pieces; a chunk is never reused (pieces keep
    its storage alive), so lifetime rules are those of ordinary tensors.  Pieces are fresh tensors on the shared
    storage, not views, so they do not share autograd version counters.  A captured graph must re-zero its
    accumulators on every replay: `capture_begin()` / `capture_end()` drop the current chunk, so every chunk used
    inside a capture is allocated -- and its ONE fill recorded -- inside that capture."""
    CHUNK = 1 << 22  # floats

    def __init__(self):
        self.buf, self.off = None, 0

    def take(self, shape, device):
        n = 1
        for d in shape:
            n *= int(d)
        n_al = (n + 63) // 64 * 64
        if n_al > self.CHUNK // 4:
            return torch.zeros(shape, device=device, dtype=f32)
        if self.buf is None or self.off + n_al > self.CHUNK or self.buf.device != device:
            self.buf, self.off = torch.zeros(self.CHUNK, device=device, dtype=f32), 0
        out = torch.empty(0, device=device, dtype=f32).set_(self.buf.untyped_storage(), self.off, tuple(shape))
        self.off += n_al
        return out


_zero_pool = _ZeroPool()


def zeros_f32(shape, device):
    return _zero_pool.take(tuple(shape), device)


def capture_begin():
    """call right before a stream capture starts (and capture_end() right after it ends)"""
    _zero_pool.buf = None
    _tables.begin()


def note_capture_pin(obj) -> bool:
    """`obj` (a weight-prep plan) is read by the graph being captured: it gets one pin (`obj.pins += 1`) that
    release_capture() of this capture's token takes back.  False when the capture runs without capture_begin() /
    capture_end() (nobody could release the pin: the caller pins for good)."""
    if not _tables.deferring:
        return False
    if not any(o is obj for o in _tables.pins):
        obj.pins += 1
        _tables.pins.append(obj)
    return True


def capture_end():
    """-> token of the launch-table slots the capture took: hand it to release_capture() when the graph is destroyed"""
    _zero_pool.buf = None
    return _tables.end()


def release_capture(token):
    """the graph captured between the capture_begin() / capture_end() that returned `token` no longer exists: its
    launch-table slots may be reused by later captures (a long-lived process that re-captures does not grow)"""
    _tables.release(token)


@contextlib.contextmanager
def capturing(graph, **kw):
    """`with capturing(g) as capture:` records the body into the torch.cuda.CUDAGraph `g` (`kw` goes to torch.cuda.graph)
    between capture_begin() and capture_end().  Afterwards `capture.token` is the token of capture_end(), to be kept with
    the graph; when the body (or the capture itself) raised, no graph came of it and the token is released here."""
    capture = types.SimpleNamespace(token=None)
    capture_begin()
    ok = False
    try:
        with torch.cuda.graph(graph, **kw):
            yield capture
        ok = True
    finally:
        capture.token = capture_end()
        if not ok:
            release_capture(capture.token)


# A cache of captured graphs is a plain dict in least-recently-used order (oldest first) whose entries carry the
# `.token` of their capture.
def drop_capture(cache: dict, key) -> None:
    """forget cache[key] and give back what its capture took"""
    ent = cache.pop(key, None)
    if ent is not None:
        torch.cuda.synchronize()            # no replay of it may still be running when its slots are reused
        release_capture(ent.token)


def lru_get(cache: dict, key):
    """cache[key], now the most recently used; None on a miss"""
    ent = cache.pop(key, None)
    if ent is not None:
        cache[key] = ent
    return ent


def lru_put(cache: dict, key, ent, limit: int) -> None:
    """insert a freshly captured entry, dropping the least recently used ones so that at most `limit` remain"""
    while len(cache) >= limit:
        drop_capture(cache, next(iter(cache)))
    cache[key] = ent


class _LaunchTables:
    """Staging for the launch tables of the grouped kernels (edm_wgrad3_group, edm_conv_wgrad_1x1_group,
    edm_wgrad_finish_multi; include/tinyedm_hip.h "LAUNCH TABLES"): the C side writes a table into host memory and it is
    copied into device memory that the kernels read -- nothing larger than a few hundred bytes travels as a by-value
    kernel argument.
    * Eager steps: (pinned host, device) slot pairs from a ring, one stream-ordered copy per table issued by the C side; a
      slot is reused only after the event recorded behind its last use has completed.
    * Between ops.capture_begin() and ops.capture_end() (graph.CapturedTrainStep): the table of a captured launch never
      changes between replays, so it is uploaded ONCE -- the C side only fills a host buffer (defer_upload), the device
      slot comes from a pool allocated up front, and capture_end() copies all of them before the first replay can run
      (no memcpy nodes in the graph: nine 4-us copies per replayed step otherwise).  capture_end() returns the slots as a
      token; release_capture(token) puts them on a free list once the graph is gone.
    * A capture made WITHOUT those hooks still works: the copy becomes a memcpy node that every replay executes again from
      the same host address, so those slots come from a bump-allocated pinned pool with ITS OWN index (`bare_i`: deferred
      captures do not eat into it), never reused or freed (allocated up front: pinning memory is not a capturable call).
    Per-device state is created by the first EAGER launch (or capture_begin()): creating it under capture would pin memory
    and hipMalloc inside the capture, so that raises instead."""
    RING, POOL = 64, 512

    def __init__(self):
        self.dev = {}
        self.deferring = False
        self.pending = []           # (device tensor, host tensor) pairs to upload at capture_end()
        self.taken = []             # (device index, slot) of the running deferred capture
        self.pins = []              # objects pinned by the running deferred capture (note_capture_pin)

    def _state(self, device):
        key = torch.device(device).index
        key = torch.cuda.current_device() if key is None else key
        st = self.dev.get(key)
        if st is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("tinyedm_amd: the launch-table pools of this device do not exist yet and cannot be "
                                   "created under stream capture (pinned + device allocations): run one eager step first, "
                                   "or bracket the capture with ops.capture_begin() / capture_end()")
            nb = max(int(_lib.call("edm_wgrad3_apply_table_bytes")), int(_lib.call("edm_conv_wgrad_1x1_group_table_bytes")),
                     int(_lib.call("edm_wgrad_finish_multi_table_bytes")), int(_lib.call("edm_skip_gate_wgrad_multi_table_bytes")),
                     int(_lib.call("edm_skip_gate_fwd_multi_table_bytes")), int(_lib.call("edm_skip_gate_bwd_multi_table_bytes")))
            nb = (nb + 255) // 256 * 256
            d = torch.device("cuda", key)
            st = self.dev[key] = {
                "key": key, "nb": nb, "i": 0, "events": [None] * self.RING,
                "host": torch.empty(self.RING, nb, dtype=torch.uint8).pin_memory(),
                "devb": torch.empty(self.RING, nb, dtype=torch.uint8, device=d),
                "pool": torch.empty(self.POOL, nb, dtype=torch.uint8).pin_memory(), "bare_i": 0,
                "bare_devb": torch.empty(self.POOL, nb, dtype=torch.uint8, device=d),
                "pool_i": 0, "free": [],
                # device slots for captured launches, allocated HERE (eagerly, ordinary memory): a buffer allocated inside a
                # capture belongs to the graph's pool and a write to it from outside the graph (the deferred upload) did
                # not reach what the replayed kernels read -- the first replay hung on a garbage table
                "pool_devb": [torch.empty(self.POOL, nb, dtype=torch.uint8, device=d)]}
        return st

    def _reserve(self, st, want):
        """make sure `want` more captured launches find a device slot -- called OUTSIDE capture (capture_begin): a process
        that holds many live graphs grows the pool instead of running out"""
        while len(st["free"]) + len(st["pool_devb"]) * self.POOL - st["pool_i"] < want:
            st["pool_devb"].append(torch.empty(self.POOL, st["nb"], dtype=torch.uint8, device=st["devb"].device))

    def take(self, device):
        """-> (host pointer, device pointer, defer_upload, release()): call release() right after the launch"""
        st = self._state(device)
        if torch.cuda.is_current_stream_capturing():
            if self.deferring:
                if st["free"]:
                    k = st["free"].pop()
                else:
                    k = st["pool_i"]
                    if k >= len(st["pool_devb"]) * self.POOL:
                        raise RuntimeError("tinyedm_amd: out of launch-table slots for this capture (more than the 64 "
                                           "reserved by ops.capture_begin(): ops._LaunchTables._reserve)")
                    st["pool_i"] = k + 1
                self.taken.append((st["key"], k))
                dev = st["pool_devb"][k // self.POOL][k % self.POOL]
                host = torch.empty(st["nb"], dtype=torch.uint8)
                self.pending.append((dev, host))
                return host.data_ptr(), dev.data_ptr(), 1, (lambda: None)
            k = st["bare_i"]
            if k >= self.POOL:
                raise RuntimeError("tinyedm_amd: out of launch-table slots for bare captures (captures made without "
                                   f"ops.capture_begin() / capture_end() share {self.POOL} pinned slots per process)")
            st["bare_i"] = k + 1                    # never reused: the graph's memcpy node keeps reading the pinned slot
            return st["pool"][k].data_ptr(), st["bare_devb"][k].data_ptr(), 0, (lambda: None)
        k = st["i"] % self.RING
        st["i"] += 1
        if st["events"][k] is not None:
            st["events"][k].synchronize()

        def release(st=st, k=k):
            ev = torch.cuda.Event()
            ev.record()
            st["events"][k] = ev
        return st["host"][k].data_ptr(), st["devb"][k].data_ptr(), 0, release

    def begin(self):
        self.deferring, self.pending, self.taken, self.pins = True, [], [], []
        if torch.cuda.is_available():
            self._reserve(self._state(torch.cuda.current_device()), 64)     # (a captured training step takes 12)

    def end(self):
        """upload the tables of the capture that just ended (their launches have only been recorded so far)"""
        pend, self.pending, self.deferring = self.pending, [], False
        taken, self.taken = tuple(self.taken), []
        pins, self.pins = tuple(self.pins), []
        for dev, host in pend:
            dev.copy_(host)
        if pend:
            torch.cuda.synchronize(pend[0][0].device)
        return _CaptureToken(taken, pins)

    def release(self, token):
        if token is None or token.released:
            return
        token.released = True
        for key, k in token.slots:
            st = self.dev.get(key)
            if st is not None and k not in st["free"]:
                st["free"].append(k)
        for obj in token.pins:          # the graph that read these plans' buffers is gone (they used to stay
            obj.pins = max(0, obj.pins - 1)   # pinned -- and their packs alive -- for the life of the Denoiser)


class _CaptureToken:
    """what a captured graph holds on to: launch-table slots and pinned weight-prep plans (ops.release_capture frees both)"""
    __slots__ = ("slots", "pins", "released")

    def __init__(self, slots, pins):
        self.slots, self.pins, self.released = slots, pins, False

    def __iter__(self):             # (round-4/5 callers iterated the token as its slot list)
        return iter(self.slots)

    def __len__(self):
        return len(self.slots)


_tables = _LaunchTables()


class GraphCorruptionError(RuntimeError):
    """raised by check_health(): a training step or a sampler solve produced non-finite values"""


_HEALTH = {}


def health(device):
    """Per-device sticky 32-bit health word.  The optimizer kernel ORs bit 0 into it when a non-finite gradient or
    weight passes through a step, the Heun update kernels bit 1 when the sampler state goes non-finite.  It is the
    in-graph sentinel of the hipGraph paths: a replay that ran with corrupted kernel arguments (tinyedm_amd/_runtime_env.py)
    leaves the bit behind, and check_health() turns it into an exception at the next host read point."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    h = _HEALTH.get(idx)
    if h is None:
        h = _HEALTH[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return h


def check_health(device, what: str):
    """Read (one host sync) and clear the health word of `device`; raise GraphCorruptionError if a bit is set."""
    h = health(device)
    v = int(h.item())
    if v:
        h.zero_()
        bits = [n for b, n in ((1, "non-finite gradient/weight in an optimizer step"), (2, "non-finite sampler state")) if v & b]
        raise GraphCorruptionError(f"{what}: {' and '.join(bits)} (health word {v:#x}).  The values computed on the GPU are "
                                   "garbage: a diverged run, NaN inputs, or a corrupted hipGraph replay "
                                   "(see tinyedm_amd/_runtime_env.py); nothing after this point can be trusted")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk(t: torch.Tensor, dtype, name: str, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA/HIP tensor -- tinyedm_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _nhwc(t, name):
    _chk(t, bf16, name)
    if t.dim() != 4:
        raise ValueError(f"{name}: expected (B,H,W,C)")
    return t.shape


# ------------------------------------------------------------------ elementwise
def pixelnorm_silu_fwd(x):
    B, H, W, C = _nhwc(x, "x")
    xn, a = torch.empty_like(x), torch.empty_like(x)
    d = torch.empty(B * H * W, device=x.device, dtype=f32)
    _lib.call("edm_pixelnorm_silu_fwd", _p(x), _p(xn), _p(a), _p(d), B * H * W, C, _stream())
    return xn, a, d


def pixelnorm_silu_bwd(xn, d, gxn, gxn_scale, ga, gadd=None):
    """gadd (optional): a gradient of the same tensor from another consumer (the U-Net skip), added in the same pass"""
    B, H, W, C = _nhwc(xn, "xn")
    _chk(d, f32, "d", (B * H * W,))
    if gxn is not None:
        _chk(gxn, bf16, "gxn", xn.shape)
    if ga is not None:
        _chk(ga, bf16, "ga", xn.shape)
    if gadd is not None:
        _chk(gadd, bf16, "gadd", xn.shape)
    gx = torch.empty_like(xn)
    _lib.call("edm_pixelnorm_silu_bwd", _p(xn), _p(d), _p(gxn), float(gxn_scale), _p(ga), _p(gadd), _p(gx), B * H * W, C,
              _stream())
    return gx


def pool_pixelnorm_silu_fwd(x):
    """(xn, a, d) of the 2x2-average-pooled x, the pooled tensor never written (== pixelnorm_silu_fwd(pool2(x)), bit for bit)"""
    B, H, W, C = _nhwc(x, "x")
    if H % 2 or W % 2 or C > 1024:
        raise ValueError("pool_pixelnorm_silu_fwd: H, W even and C <= 1024 required")
    xn = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=bf16)
    a = torch.empty_like(xn)
    d = torch.empty(B * (H // 2) * (W // 2), device=x.device, dtype=f32)
    _lib.call("edm_pool_pixelnorm_silu_fwd", _p(x), _p(xn), _p(a), _p(d), B, H // 2, W // 2, C, _stream())
    return xn, a, d


def pool_pixelnorm_silu_bwd(xn, d, gxn, gxn_scale, ga, gadd=None):
    """backward of pool_pixelnorm_silu_fwd: the gradient w.r.t. the tensor BEFORE the pool, (B, 2H, 2W, C); gadd (optional, that
    shape): a gradient of the same tensor from another consumer (the U-Net skip) (== up2(pixelnorm_silu_bwd(...), 0.25, add=gadd))"""
    B, H, W, C = _nhwc(xn, "xn")
    _chk(d, f32, "d", (B * H * W,))
    if gxn is not None:
        _chk(gxn, bf16, "gxn", xn.shape)
    if ga is not None:
        _chk(ga, bf16, "ga", xn.shape)
    if gadd is not None:
        _chk(gadd, bf16, "gadd", (B, 2 * H, 2 * W, C))
    gx = torch.empty(B, 2 * H, 2 * W, C, device=xn.device, dtype=bf16)
    _lib.call("edm_pool_pixelnorm_silu_bwd", _p(xn), _p(d), _p(gxn), float(gxn_scale), _p(ga), _p(gadd), _p(gx), B, H, W, C,
              _stream())
    return gx


def up2_silu(x):
    """(y, a): y = nearest-exact x2 upsample of x, a = mp_silu(y), one pass"""
    B, H, W, C = _nhwc(x, "x")
    y = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=bf16)
    a = torch.empty_like(y)
    _lib.call("edm_up2_silu", _p(x), _p(y), _p(a), B, 2 * H, 2 * W, C, _stream())
    return y, a


def silu_fwd(x):
    _chk(x, bf16, "x")
    a = torch.empty_like(x)
    _lib.call("edm_silu_fwd", _p(x), _p(a), x.numel(), _stream())
    return a


def silu_bwd(x, ga, gextra=None, extra_scale=1.0):
    _chk(x, bf16, "x")
    _chk(ga, bf16, "ga", x.shape)
    if gextra is not None:
        _chk(gextra, bf16, "gextra", x.shape)
    gx = torch.empty_like(x)
    _lib.call("edm_silu_bwd", _p(x), _p(ga), _p(gextra), float(extra_scale), _p(gx), x.numel(), _stream())
    return gx


def axpby(a, alpha, b=None, beta=0.0):
    _chk(a, bf16, "a")
    if b is not None:
        _chk(b, bf16, "b", a.shape)
    out = torch.empty_like(a)
    _lib.call("edm_axpby", _p(a), float(alpha), _p(b), float(beta), _p(out), a.numel(), _stream())
    return out


def _lin_view(lin, B, C, name):
    """(B, C) fp32 view whose rows may be strided (a column slice of the batched embed-linear output)."""
    if not lin.is_cuda or lin.dtype != f32 or lin.dim() != 2 or tuple(lin.shape) != (B, C) or lin.stride(1) != 1:
        raise ValueError(f"{name}: expected a (B={B}, C={C}) fp32 GPU tensor with unit column stride")
    if lin.stride(0) < C:
        raise ValueError(f"{name}: row stride {lin.stride(0)} < C={C}")
    return lin.stride(0)


def _dyn(dyn):
    """device edm_step_params record (48 bytes) or None"""
    if dyn is None:
        return None
    if not dyn.is_cuda or dyn.numel() * dyn.element_size() < 48 or not dyn.is_contiguous():
        raise ValueError("dyn: expected a contiguous device buffer of >= 48 bytes (edm_step_params)")
    return ctypes.c_void_p(dyn.data_ptr())


def mod_silu_drop_fwd(r, lin, gain, pdrop, seed, sub, step, dyn=None):
    B, H, W, C = _nhwc(r, "r")
    ls = _lin_view(lin, B, C, "lin")
    _chk(gain, f32, "gain")
    a = torch.empty_like(r)
    _lib.call("edm_mod_silu_drop_fwd", _p(r), _p(lin), ls, _p(gain), _p(a), B, H * W, C, float(pdrop), int(seed), int(sub),
              int(step), _dyn(dyn), _stream())
    return a


def mod_silu_drop_bwd(r, lin, gain, ga, pdrop, seed, sub, step, glin_out=None, ggain_out=None, dyn=None, gm_out=None):
    """glin_out: optional (B, C) strided fp32 view to receive d loss / d lin (else a fresh tensor);
    ggain_out: optional 0-dim fp32 tensor that d loss / d gain is ACCUMULATED into (else a fresh zero scalar).
    gm_out: a zero-filled (B, C) fp32 view with unit column stride (a column slice of the buffer all blocks share): the raw
    modulation gradient is accumulated there and NOT finished -- returns (gr, None, None); one mod_finish_multi over the
    shared buffer finishes every block (as conv3x3_modbwd(gm_out=...))."""
    B, H, W, C = _nhwc(r, "r")
    ls = _lin_view(lin, B, C, "lin")
    _chk(ga, bf16, "ga", r.shape)
    gr = torch.empty_like(r)
    if gm_out is not None:
        gms = _lin_view(gm_out, B, C, "gm_out")
        _chk(gain, f32, "gain")
        _lib.call("edm_mod_silu_drop_bwd_raw", _p(r), _p(lin), ls, _p(gain), _p(ga), _p(gr), _p(gm_out), gms, B, H * W, C,
                  float(pdrop), int(seed), int(sub), int(step), _dyn(dyn), _stream())
        return gr, None, None
    gm = zeros_f32((B, C), r.device)
    glin = torch.empty(B, C, device=r.device, dtype=f32) if glin_out is None else glin_out
    gs = _lin_view(glin, B, C, "glin")
    ggain = zeros_f32((), r.device) if ggain_out is None else _chk(ggain_out, f32, "ggain_out", ())
    _lib.call("edm_mod_silu_drop_bwd", _p(r), _p(lin), ls, _p(gain), _p(ga), _p(gr), _p(gm), _p(glin), gs, _p(ggain), B,
              H * W, C, float(pdrop), int(seed), int(sub), int(step), _dyn(dyn), _stream())
    return gr, glin, ggain


def dropout_mask(n, pdrop, seed, sub, step, device):
    m = torch.empty(n, device=device, dtype=torch.uint8)
    _lib.call("edm_dropout_mask", _p(m), n, float(pdrop), int(seed), int(sub), int(step), _stream())
    return m


def pool2(x, scale=0.25):
    B, H, W, C = _nhwc(x, "x")
    if H % 2 or W % 2:
        raise ValueError("pool2: H and W must be even")
    y = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=bf16)
    _lib.call("edm_pool2", _p(x), _p(y), B, H // 2, W // 2, C, float(scale), _stream())
    return y


def up2(x, scale=1.0, add=None):
    """y = scale * nearest-exact x2 upsample of x (+ add, a bf16 tensor of the output shape)"""
    B, H, W, C = _nhwc(x, "x")
    if add is not None:
        _chk(add, bf16, "add", (B, 2 * H, 2 * W, C))
    y = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=bf16)
    _lib.call("edm_up2", _p(x), _p(add), _p(y), B, 2 * H, 2 * W, C, float(scale), _stream())
    return y


def reduce_hw(x, C=None, c_off=0, y=None, scale=1.0):
    """out[b,c] = scale * sum_hw x[b,hw,c_off+c] (* y[b,hw,c])."""
    B, H, W, Cx = _nhwc(x, "x")
    C = Cx - c_off if C is None else C
    if c_off % 8 or c_off + C > Cx:
        raise ValueError("reduce_hw: bad channel slice")
    out = torch.empty(B, C, device=x.device, dtype=f32)      # written (not accumulated) in a fixed summation order
    ys = 0
    if y is not None:
        By, Hy, Wy, Cy = _nhwc(y, "y")
        if (By, Hy, Wy) != (B, H, W) or Cy < C:
            raise ValueError("reduce_hw: y shape mismatch")
        ys = Cy
    xp = ctypes.c_void_p(x.data_ptr() + 2 * c_off)
    _lib.call("edm_reduce_hw", xp, Cx, _p(y), ys, _p(out), B, H * W, C, float(scale), _stream())
    return out


def scalelong_fwd(mean, w1h, w2h):
    B, C = mean.shape
    R = w1h.shape[0]
    _chk(mean, f32, "mean")
    _chk(w1h, f32, "w1h", (R, C + 1))
    _chk(w2h, f32, "w2h", (C, R))
    gate = torch.empty(B, C, device=mean.device, dtype=f32)
    z1 = torch.empty(B, R, device=mean.device, dtype=f32)
    _lib.call("edm_scalelong_fwd", _p(mean), _p(w1h), _p(w2h), _p(gate), _p(z1), B, C, R, _stream())
    return gate, z1


def scalelong_bwd(mean, w1h, w2h, gate, z1, ggate):
    B, C = mean.shape
    R = w1h.shape[0]
    _chk(ggate, f32, "ggate", (B, C))
    gmean = torch.empty(B, C, device=mean.device, dtype=f32)
    gw1 = zeros_f32(w1h.shape, w1h.device)
    gw2 = zeros_f32(w2h.shape, w2h.device)
    _lib.call("edm_scalelong_bwd", _p(mean), _p(w1h), _p(w2h), _p(gate), _p(z1), _p(ggate), _p(gmean), _p(gw1), _p(gw2),
              B, C, R, _stream())
    return gmean, gw1, gw2


def skip_gate_fwd(skip, w1h, w2h):
    """ScaleLong gate of a skip tensor in one launch: (mean (B,C), gate (B,C), z1 (B,R)) == reduce_hw(skip)/HW followed by
    scalelong_fwd."""
    B, H, W, C = _nhwc(skip, "skip")
    R = w1h.shape[0]
    _chk(w1h, f32, "w1h", (R, C + 1))
    _chk(w2h, f32, "w2h", (C, R))
    mean = torch.empty(B, C, device=skip.device, dtype=f32)
    gate = torch.empty(B, C, device=skip.device, dtype=f32)
    z1 = torch.empty(B, R, device=skip.device, dtype=f32)
    _lib.call("edm_skip_gate_fwd", _p(skip), _p(w1h), _p(w2h), _p(mean), _p(gate), _p(z1), B, H * W, C, R, _stream())
    return mean, gate, z1


def skip_gate_fwd_multi(items):
    """skip_gate_fwd for several skip tensors of ONE channel count in one launch: items = sequence (<= 32) of
    (skip, w1h, w2h) or (skip, w1h, w2h, cat, sil) -> list of (mean, gate, z1), the values of the per-tensor call.
    cat / sil: (B, H, W, Ci + C) contiguous bf16 buffers whose right C columns receive skip * gate and mp_silu of it
    (== skip_half_fwd(skip, gate, cat, sil), by the workgroup that just reduced the sample)."""
    n = len(items)
    if not 0 < n <= 32:
        raise ValueError("skip_gate_fwd_multi: 1..32 gates per launch")
    arr = (_lib.SkipGateFwdItem * n)()
    out = []
    C0 = items[0][0].shape[-1]
    for k, item in enumerate(items):
        skip, w1h, w2h = item[:3]
        cat, sil = item[3:5] if len(item) > 3 else (None, None)
        B, H, W, C = _nhwc(skip, "skip")
        Ci = 0
        if cat is not None:
            Ci = cat.shape[-1] - C
            _chk(cat, bf16, "cat", (B, H, W, Ci + C))
            if sil is not None:
                _chk(sil, bf16, "sil", (B, H, W, Ci + C))
            if Ci <= 0 or Ci % 8:
                raise ValueError("skip_gate_fwd_multi: cat must have Ci + C channels with Ci a positive multiple of 8")
        elif sil is not None:
            raise ValueError("skip_gate_fwd_multi: sil needs cat")
        if C != C0:
            raise ValueError("skip_gate_fwd_multi: the gates of one launch share a channel count")
        R = w1h.shape[0]
        _chk(w1h, f32, "w1h", (R, C + 1))
        _chk(w2h, f32, "w2h", (C, R))
        mean = torch.empty(B, C, device=skip.device, dtype=f32)
        gate = torch.empty(B, C, device=skip.device, dtype=f32)
        z1 = torch.empty(B, R, device=skip.device, dtype=f32)
        arr[k] = _lib.SkipGateFwdItem(skip.data_ptr(), w1h.data_ptr(), w2h.data_ptr(), mean.data_ptr(), gate.data_ptr(),
                                      z1.data_ptr(), _p(cat), _p(sil), B, H * W, C, R, Ci, 0)
        out.append((mean, gate, z1))
    th, td, defer, release = _tables.take(items[0][0].device)
    _lib.call("edm_skip_gate_fwd_multi", ctypes.byref(arr), n, ctypes.c_void_p(th), ctypes.c_void_p(td), defer, _stream())
    release()
    return out


def skip_gate_bwd_multi(items):
    """the per-sample pass of skip_gate_bwd(defer_wgrad=True) for several gates of ONE channel count in one launch:
    items = sequence (<= 32) of (gcat, Ci, skip, w1h, w2h, gate, z1[, gskip]) -> list of (gmean (B, C), ws (B, C + 2R)).
    gskip: an uninitialised (B, H, W, C) bf16 tensor that receives gcat[..., Ci:] * gate + gmean / HW (== skip_half_bwd), written
    by the workgroup that just reduced the sample."""
    n = len(items)
    if not 0 < n <= 32:
        raise ValueError("skip_gate_bwd_multi: 1..32 gates per launch")
    arr = (_lib.SkipGateBwdItem * n)()
    out = []
    C0 = items[0][2].shape[-1]
    for k, item in enumerate(items):
        gcat, Ci, skip, w1h, w2h, gate, z1 = item[:7]
        gskip = item[7] if len(item) > 7 else None
        B, H, W, Ct = _nhwc(gcat, "gcat")
        Bs, Hs, Ws, C = _nhwc(skip, "skip")
        if (Bs, Hs, Ws) != (B, H, W) or Ct != Ci + C or C != C0:
            raise ValueError("skip_gate_bwd_multi: gcat/skip shape mismatch, or mixed channel counts in one launch")
        R = w1h.shape[0]
        _chk(w1h, f32, "w1h", (R, C + 1))
        _chk(w2h, f32, "w2h", (C, R))
        _chk(gate, f32, "gate", (B, C))
        _chk(z1, f32, "z1", (B, R))
        gmean = torch.empty(B, C, device=skip.device, dtype=f32)
        ws = torch.empty(B, C + 2 * R, device=skip.device, dtype=f32)
        if gskip is not None:
            _chk(gskip, bf16, "gskip", (B, H, W, C))
        arr[k] = _lib.SkipGateBwdItem(gcat.data_ptr(), Ct, skip.data_ptr(), w1h.data_ptr(), w2h.data_ptr(), gate.data_ptr(),
                                      z1.data_ptr(), gmean.data_ptr(), ws.data_ptr(), _p(gskip), Ci, B, H * W, C, R, 0)
        out.append((gmean, ws))
    th, td, defer, release = _tables.take(items[0][2].device)
    _lib.call("edm_skip_gate_bwd_multi", ctypes.byref(arr), n, ctypes.c_void_p(th), ctypes.c_void_p(td), defer, _stream())
    release()
    return out


def skip_half_bwd_multi(items):
    """skip_half_bwd for several tensors in one launch: items = sequence (<= 32) of (gcs, gate, gmean, gskip) with gskip an
    uninitialised tensor like gcs that is WRITTEN (the caller handed it out earlier as a placeholder)."""
    n = len(items)
    if not 0 < n <= 32:
        raise ValueError("skip_half_bwd_multi: 1..32 tensors per launch")
    arr = (_lib.SkipHalfBwdItem * n)()
    for k, (gcs, gate, gmean, gskip) in enumerate(items):
        B, H, W, Cs = _nhwc(gcs, "gcs")
        _chk(gate, f32, "gate", (B, Cs))
        _chk(gmean, f32, "gmean", (B, Cs))
        _chk(gskip, bf16, "gskip", (B, H, W, Cs))
        arr[k] = _lib.SkipHalfBwdItem(gcs.data_ptr(), gate.data_ptr(), gmean.data_ptr(), gskip.data_ptr(), B, H * W, Cs, 0)
    th, td, defer, release = _tables.take(items[0][0].device)
    _lib.call("edm_skip_half_bwd_multi", ctypes.byref(arr), n, ctypes.c_void_p(th), ctypes.c_void_p(td), defer, _stream())
    release()


def skip_gate_bwd(gcat, Ci, skip, mean, w1h, w2h, gate, z1, defer_wgrad=False):
    """backward of skip_gate_fwd given the gradient of cat = [inp, skip*gate]: (gmean, gw1h, gw2h) == reduce_hw(gcat[...,
    Ci:] * skip) followed by scalelong_bwd.  defer_wgrad=True: -> (gmean, ws): the batch sums that form gw1h / gw2h are left
    to ONE skip_gate_wgrad_multi over every gate of the backward pass (ws = this gate's per-sample vectors)."""
    B, H, W, Ct = _nhwc(gcat, "gcat")
    Bs, Hs, Ws, C = _nhwc(skip, "skip")
    if (Bs, Hs, Ws) != (B, H, W) or Ci + C != Ct or Ci % 8:
        raise ValueError("skip_gate_bwd: gcat / skip shape mismatch")
    R = w1h.shape[0]
    _chk(mean, f32, "mean", (B, C))
    _chk(gate, f32, "gate", (B, C))
    _chk(z1, f32, "z1", (B, R))
    _chk(w1h, f32, "w1h", (R, C + 1))
    _chk(w2h, f32, "w2h", (C, R))
    gmean = torch.empty(B, C, device=skip.device, dtype=f32)
    gw1 = None if defer_wgrad else torch.empty(w1h.shape, device=w1h.device, dtype=f32)
    gw2 = None if defer_wgrad else torch.empty(w2h.shape, device=w2h.device, dtype=f32)
    ws = torch.empty(B, C + 2 * R, device=skip.device, dtype=f32)
    _lib.call("edm_skip_gate_bwd", _p(gcat), Ct, Ci, _p(skip), _p(mean), _p(w1h), _p(w2h), _p(gate), _p(z1), _p(gmean),
              _p(gw1), _p(gw2), _p(ws), B, H * W, C, R, _stream())
    return (gmean, ws) if defer_wgrad else (gmean, gw1, gw2)


def skip_gate_wgrad_multi(items):
    """items: sequence (<= 32) of (ws, mean, R) from skip_gate_bwd(defer_wgrad=True) and the gate's forward -> list of
    (gw1h (R, C+1), gw2h (C, R)), all from ONE launch"""
    n = len(items)
    if not 0 < n <= 32:
        raise ValueError("skip_gate_wgrad_multi: 1..32 gates per launch")
    arr = (_lib.SkipGateWgradItem * n)()
    out = []
    for k, (ws, mean, R) in enumerate(items):
        _chk(mean, f32, "mean")
        B, C = mean.shape
        _chk(ws, f32, "ws", (B, C + 2 * R))
        gw1 = torch.empty(R, C + 1, device=ws.device, dtype=f32)
        gw2 = torch.empty(C, R, device=ws.device, dtype=f32)
        arr[k] = _lib.SkipGateWgradItem(ws.data_ptr(), mean.data_ptr(), gw1.data_ptr(), gw2.data_ptr(), B, C, R, 0)
        out.append((gw1, gw2))
    th, td, defer, release = _tables.take(items[0][0].device)
    _lib.call("edm_skip_gate_wgrad_multi", ctypes.byref(arr), n, ctypes.c_void_p(th), ctypes.c_void_p(td), defer, _stream())
    release()
    return out


def concat_gate_fwd(inp, skip, gate, want_silu):
    B, H, W, Ci = _nhwc(inp, "inp")
    Bs, Hs, Ws, Cs = _nhwc(skip, "skip")
    if (Bs, Hs, Ws) != (B, H, W):
        raise ValueError("concat_gate_fwd: inp/skip spatial mismatch")
    _chk(gate, f32, "gate", (B, Cs))
    cat = torch.empty(B, H, W, Ci + Cs, device=inp.device, dtype=bf16)
    sil = torch.empty_like(cat) if want_silu else None
    _lib.call("edm_concat_gate_fwd", _p(inp), _p(skip), _p(gate), _p(cat), _p(sil), B, H * W, Ci, Cs, _stream())
    return cat, sil


def concat_gate_bwd(gcat, gate, gmean, Ci):
    B, H, W, Ct = _nhwc(gcat, "gcat")
    Cs = Ct - Ci
    _chk(gate, f32, "gate", (B, Cs))
    _chk(gmean, f32, "gmean", (B, Cs))
    ginp = torch.empty(B, H, W, Ci, device=gcat.device, dtype=bf16)
    gskip = torch.empty(B, H, W, Cs, device=gcat.device, dtype=bf16)
    _lib.call("edm_concat_gate_bwd", _p(gcat), _p(gate), _p(gmean), _p(ginp), _p(gskip), B, H * W, Ci, Cs, _stream())
    return ginp, gskip


def skip_half_fwd(skip, gate, cat, sil=None):
    """cat[..., Ci:] = skip*gate (and sil[..., Ci:] = mp_silu of it) in place: the skip half of the decoder's concatenated
    operands; the input half was written by the producer of `input` (conv_igemm(out=, silu_out=))."""
    B, H, W, Cs = _nhwc(skip, "skip")
    _chk(gate, f32, "gate", (B, Cs))
    Ct = cat.shape[-1]
    _chk(cat, bf16, "cat", (B, H, W, Ct))
    if sil is not None:
        _chk(sil, bf16, "sil", (B, H, W, Ct))
    if Ct <= Cs:
        raise ValueError("skip_half_fwd: cat must be wider than the skip")
    _lib.call("edm_skip_half_fwd", _p(skip), _p(gate), _p(cat), _p(sil), B, H * W, Ct - Cs, Cs, _stream())


def skip_half_bwd(gcs, gate, gmean):
    """gskip = gcs*gate + gmean/HW from the skip half gcs of d loss / d cat (conv_igemm(split=) wrote it)"""
    B, H, W, Cs = _nhwc(gcs, "gcs")
    _chk(gate, f32, "gate", (B, Cs))
    _chk(gmean, f32, "gmean", (B, Cs))
    gskip = torch.empty_like(gcs)
    _lib.call("edm_skip_half_bwd", _p(gcs), _p(gate), _p(gmean), _p(gskip), B, H * W, Cs, _stream())
    return gskip


def _sigma_arg(sigma, B):
    _chk(sigma, f32, "sigma")
    if sigma.numel() == 1:
        return 0
    if sigma.numel() != B:
        raise ValueError(f"sigma must have 1 or {B} elements, got {sigma.numel()}")
    return 1


def precond_in(noisy, sigma, sigma_data, CP):
    _chk(noisy, f32, "noisy")
    B, Cimg, H, W = noisy.shape
    ss = _sigma_arg(sigma, B)
    out = torch.empty(B, H, W, CP, device=noisy.device, dtype=bf16)
    _lib.call("edm_precond_in", _p(noisy), _p(sigma), ss, float(sigma_data), _p(out), B, Cimg, H * W, CP, _stream())
    return out


def conv_out_fwd(x, w_hat, gain_out, noisy, sigma, sigma_data, want_fraw=True):
    B, H, W, C = _nhwc(x, "x")
    Co = w_hat.shape[0]
    _chk(w_hat, f32, "w_hat", (Co, C))
    _chk(noisy, f32, "noisy", (B, Co, H, W))
    _chk(gain_out, f32, "gain_out")
    ss = _sigma_arg(sigma, B)
    D = torch.empty(B, Co, H, W, device=x.device, dtype=f32)
    Fraw = torch.empty(B, Co, H, W, device=x.device, dtype=f32) if want_fraw else None
    _lib.call("edm_conv_out_fwd", _p(x), _p(w_hat), _p(gain_out), _p(noisy), _p(sigma), ss, float(sigma_data), _p(D),
              _p(Fraw), B, H * W, C, Co, _stream())
    return D, Fraw


def conv_out_bwd(x, w_hat, gain_out, Fraw, dD, sigma, sigma_data, gg_out=None):
    """gg_out: optional 0-dim fp32 tensor that d loss / d gain_out is ACCUMULATED into (else a fresh zero scalar)"""
    B, H, W, C = _nhwc(x, "x")
    Co = w_hat.shape[0]
    _chk(dD, f32, "dD", (B, Co, H, W))
    _chk(Fraw, f32, "Fraw", (B, Co, H, W))
    ss = _sigma_arg(sigma, B)
    gx = torch.empty_like(x)
    gw = zeros_f32(w_hat.shape, w_hat.device)
    gg = zeros_f32((), x.device) if gg_out is None else _chk(gg_out, f32, "gg_out", ())
    _lib.call("edm_conv_out_bwd", _p(x), _p(w_hat), _p(gain_out), _p(Fraw), _p(dD), _p(sigma), ss, float(sigma_data),
              _p(gx), _p(gw), _p(gg), B, H * W, C, Co, _stream())
    return gx, gw, gg


def conv_out_bwd_x(w_hat, gain_out, dD, sigma, sigma_data, C):
    """the input gradient of conv_out alone (bf16 NHWC); the weight / gain gradients come from lowrank_wgrad"""
    Co = w_hat.shape[0]
    _chk(w_hat, f32, "w_hat", (Co, C))
    _chk(dD, f32, "dD")
    B, _, H, W = dD.shape
    ss = _sigma_arg(sigma, B)
    gx = torch.empty(B, H, W, C, device=dD.device, dtype=bf16)
    _lib.call("edm_conv_out_bwd", None, _p(w_hat), _p(gain_out), None, _p(dD), _p(sigma), ss, float(sigma_data),
              _p(gx), None, None, B, H * W, C, Co, _stream())
    return gx


# ------------------------------------------------------------------ the output end in factored form (csrc/tail_lowrank.hip)
LOWRANK_MAX_CO = 8


@functools.lru_cache(maxsize=None)
def lowrank_supported(C, Co, W, taps):
    """the factored kernels run this shape (their LDS tables fit): lowrank_wgrad(taps) and, taps == 9, lowrank_dgrad3x3_modbwd.
    A host query, not a launch (_lib.N_CALLS)."""
    return bool(_lib.lib().edm_lowrank_supported(int(C), int(Co), int(W), int(taps)))


def lowrank_df(dD, Fraw, gain_out, sigma, sigma_data, want_aux=True):
    """dF = dD * c_out * gain_out (fp32 NCHW, the rank-Co factor of conv_out's input gradient) and, want_aux,
    aux = dD * c_out * Fraw, whose sum is d loss / d gain_out"""
    _chk(dD, f32, "dD")
    B, Co, H, W = dD.shape
    ss = _sigma_arg(sigma, B)
    _chk(gain_out, f32, "gain_out")
    dF = torch.empty_like(dD)
    aux = None
    if want_aux:
        _chk(Fraw, f32, "Fraw", dD.shape)
        aux = torch.empty_like(dD)
    _lib.call("edm_lowrank_df", _p(dD), _p(Fraw), _p(gain_out), _p(sigma), ss, float(sigma_data), _p(dF), _p(aux), B, Co,
              H * W, _stream())
    return dF, aux


def _lowrank_args(dF, Wc, C):
    _chk(dF, f32, "dF")
    if dF.dim() != 4 or not 1 <= dF.shape[1] <= LOWRANK_MAX_CO:
        raise ValueError(f"dF: expected (B, Co <= {LOWRANK_MAX_CO}, H, W)")
    B, Co, H, W = dF.shape
    _chk(Wc, f32, "Wc", (Co, 9, C))
    return B, Co, H, W


def lowrank_dgrad3x3(dF, Wc, scale=1.0):
    """ga2 (bf16 NHWC [B, H, W, C]) = scale * sum_t sum_o dF[p - d(t), o] * Wc[o, t, :]: the dgrad of a 3x3 conv whose
    output gradient is dF . Wout, from the Co-channel factor dF (fp32 NCHW) and Wc = lowrank_expand_wc(Wout, dgrad pack)"""
    C = Wc.shape[-1]
    B, Co, H, W = _lowrank_args(dF, Wc, C)
    ga = torch.empty(B, H, W, C, device=dF.device, dtype=bf16)
    _lib.call("edm_lowrank_dgrad3x3", _p(dF), _p(Wc), float(scale), _p(ga), None, None, 0, None, None, None, 0, 0.0, 0, 0, 0,
              0, B, H, W, C, Co, None, _stream())
    return ga


def lowrank_dgrad3x3_modbwd(dF, Wc, alpha, r1, lin, gain, pdrop, seed, sub, step, glin_out=None, ggain_out=None, dyn=None,
                            gm_out=None, u_marked=False):
    """lowrank_dgrad3x3 with the modulation backward on its result in registers: conv3x3_modbwd (same arguments, same
    returns) for an output gradient of rank Co; no constraint on H * W"""
    B, H, W, C = _nhwc(r1, "r1")
    if tuple(dF.shape[0:1] + dF.shape[2:]) != (B, H, W):
        raise ValueError(f"lowrank_dgrad3x3_modbwd: dF {tuple(dF.shape)} does not match r1 {tuple(r1.shape)}")
    _, Co, _, _ = _lowrank_args(dF, Wc, C)
    ls = _lin_view(lin, B, C, "lin")
    _chk(gain, f32, "gain")
    gr = torch.empty_like(r1)
    if gm_out is not None:
        gms = _lin_view(gm_out, B, C, "gm_out")
        gm = gm_out
    else:
        gms = C
        gm = zeros_f32((B, C), r1.device)
        glin = torch.empty(B, C, device=r1.device, dtype=f32) if glin_out is None else glin_out
        gs = _lin_view(glin, B, C, "glin")
        ggain = zeros_f32((), r1.device) if ggain_out is None else _chk(ggain_out, f32, "ggain_out", ())
    _lib.call("edm_lowrank_dgrad3x3", _p(dF), _p(Wc), float(alpha), None, _p(r1), _p(lin), ls, _p(gain), _p(gr), _p(gm),
              gms, float(pdrop), int(seed), int(sub), int(step), int(bool(u_marked)), B, H, W, C, Co, _dyn(dyn), _stream())
    if gm_out is not None:
        return gr, None, None
    _lib.call("edm_mod_finish", _p(gm), _p(lin), ls, _p(gain), _p(glin), gs, _p(ggain), B, C, _stream())
    return gr, glin, ggain


def lowrank_wgrad(dF, X, taps, aux=None, aux_out=None):
    """G (fp32 [Co, taps, C]) = sum_p dF[p, o] * X[p + d(t), c] (X bf16 NHWC, taps 1 or 9), deterministic.  aux (fp32 like
    dF): its sum is ACCUMULATED into the 0-dim fp32 tensor aux_out (else into a fresh zero scalar).  Returns (G, aux sum)."""
    B, H, W, C = _nhwc(X, "X")
    _chk(dF, f32, "dF")
    if dF.dim() != 4 or tuple(dF.shape[0:1] + dF.shape[2:]) != (B, H, W) or not 1 <= dF.shape[1] <= LOWRANK_MAX_CO:
        raise ValueError(f"lowrank_wgrad: dF {tuple(dF.shape)} does not match X {tuple(X.shape)}")
    if taps not in (1, 9):
        raise ValueError("lowrank_wgrad: taps must be 1 or 9")
    Co = dF.shape[1]
    asum = None
    if aux is not None:
        _chk(aux, f32, "aux", dF.shape)
        asum = zeros_f32((), X.device) if aux_out is None else _chk(aux_out, f32, "aux_out", ())
    G = torch.empty(Co, taps, C, device=X.device, dtype=f32)
    nws = int(_lib.call("edm_lowrank_wgrad_workspace", C, Co, taps))
    ws = torch.empty(nws, device=X.device, dtype=f32)
    _lib.call("edm_lowrank_wgrad", _p(dF), _p(X), int(taps), _p(aux), _p(G), _p(asum), _p(ws), nws, B, H, W, C, Co, _stream())
    return G, asum


def lowrank_expand_wc(wout_hat, wd):
    """Wc (fp32 [Co, taps, I]) = Wout_hat . float(W) from the plain bf16 dgrad pack wd [taps, I, O] of the conv (the values
    its MFMA dgrad multiplies; taps flipped back)"""
    _chk(wd, bf16, "wd")
    if wd.dim() != 3 or getattr(wd, "_edm_frag", False):
        raise ValueError("lowrank_expand_wc: expected a plain (taps, I, O) dgrad pack")
    taps, I, O = wd.shape
    Co = wout_hat.shape[0]
    _chk(wout_hat, f32, "wout_hat", (Co, O))
    Wc = torch.empty(Co, taps, I, device=wd.device, dtype=f32)
    _lib.call("edm_lowrank_expand_wc", _p(wout_hat), _p(wd), _p(Wc), Co, O, I, taps, _stream())
    return Wc


def lowrank_expand_slab(wout_hat, G, scale=1.0, Ipad=None):
    """one weight-gradient slab (1, taps, O, Ipad) fp32 in packed order, slab[t, c, i] = scale * sum_o Wout_hat[o, c] * G[o, t, i]:
    what wgrad_finish / wgrad_finish_multi / finish_grad reduce and project like any other"""
    _chk(G, f32, "G")
    Co, taps, I = G.shape
    O = wout_hat.shape[1]
    _chk(wout_hat, f32, "wout_hat", (Co, O))
    Ipad = I if Ipad is None else Ipad
    slab = torch.empty(1, taps, O, Ipad, device=G.device, dtype=f32)
    _lib.call("edm_lowrank_expand_slab", _p(wout_hat), _p(G), _p(slab), float(scale), Co, O, I, Ipad, taps, _stream())
    return slab


@functools.lru_cache(maxsize=None)
def lowrank_tail_supported(C, Cc, Co, W):
    """lowrank_tail_fwd runs maps of width W (a2 with C channels, cat with Cc, Co outputs): its LDS tables fit.  A host
    query, not a launch."""
    return bool(_lib.lib().edm_lowrank_tail_supported(int(C), int(Cc), int(Co), int(W)))


def lowrank_tail_fwd(a2, cat, Wc, Wp, sb, sa, gain_out, noisy, sigma, sigma_data, want_fraw=True):
    """(D, Fraw) of conv_out_fwd for the block output h = sb * conv3x3(a2, W2) + sa * conv1x1(cat, W1) that is never formed:
    Fraw = sb * conv3x3(a2, Wc) + sa * cat . Wp with Wc = lowrank_expand_wc(Wout_hat, dgrad pack of the 3x3 conv) and
    Wp (fp32 [Co, Cc]) = Wout_hat . W1, or Wout_hat when the block has no 1x1 conv.  Deterministic."""
    B, H, W, C = _nhwc(a2, "a2")
    Cc = cat.shape[-1]
    _chk(cat, bf16, "cat", (B, H, W, Cc))
    Co = Wc.shape[0]
    _chk(Wc, f32, "Wc", (Co, 9, C))
    _chk(Wp, f32, "Wp", (Co, Cc))
    _chk(noisy, f32, "noisy", (B, Co, H, W))
    _chk(gain_out, f32, "gain_out")
    ss = _sigma_arg(sigma, B)
    D = torch.empty(B, Co, H, W, device=a2.device, dtype=f32)
    Fraw = torch.empty(B, Co, H, W, device=a2.device, dtype=f32) if want_fraw else None
    _lib.call("edm_lowrank_tail_fwd", _p(a2), _p(cat), _p(Wc), _p(Wp), float(sb), float(sa), _p(gain_out), _p(noisy),
              _p(sigma), ss, float(sigma_data), _p(D), _p(Fraw), B, H, W, C, Cc, Co, _stream())
    return D, Fraw


def lowrank_tail_dwout_supported(C, Cc, Co, has1):
    return bool(_lib.lib().edm_lowrank_tail_dwout_supported(int(C), int(Cc), int(Co), int(bool(has1))))


def lowrank_tail_dwout(G, wf2, G1, wf1, sb, sa):
    """conv_out's weight gradient (fp32 [Co, C], before the projection through its normalisation) without the block output:
    sb * sum_{t, ci} W2[c, ci, t] G[o, t, ci] + sa * sum_cj W1[c, cj] G1[o, cj]; wf2 / wf1 = the plain bf16 forward packs
    (taps, O, I) of the block's second 3x3 conv and of its 1x1 conv (None: the block has none, + sa * G1[o, c])."""
    _chk(G, f32, "G")
    Co, _, C = G.shape
    _chk(G, f32, "G", (Co, 9, C))
    if wf2.dim() != 3 or getattr(wf2, "_edm_frag", False):
        raise ValueError("lowrank_tail_dwout: expected a plain (9, O, I) forward pack")
    _chk(wf2, bf16, "wf2", (9, C, C))
    Cc = G1.shape[-1]
    _chk(G1, f32, "G1", (Co, 1, Cc))
    if wf1 is not None:
        _chk(wf1, bf16, "wf1", (1, C, Cc))
    elif Cc != C:
        raise ValueError("lowrank_tail_dwout: without a 1x1 pack G1 must have the block's channel count")
    gwh = torch.empty(Co, C, device=G.device, dtype=f32)
    _lib.call("edm_lowrank_tail_dwout", _p(G), _p(wf2), _p(G1), _p(wf1), float(sb), float(sa), _p(gwh), Co, C, Cc, _stream())
    return gwh


def lowrank_gcat_supported(Cc, Ci, Co):
    return bool(_lib.lib().edm_lowrank_gcat_supported(int(Cc), int(Ci), int(Co)))


def lowrank_gcat_add(dF, Wp, sa, t, Ci=None):
    """d loss / d cat of the last block without conv_out's input gradient: bf16(t + sa * dF^T Wp), t (bf16 NHWC) the dense
    part.  Ci: the split of conv_igemm(split=): returns (gu [.., Ci], gcs [.., Cc - Ci]); None: (the whole gradient, None)."""
    B, H, W, Cc = _nhwc(t, "t")
    _chk(dF, f32, "dF")
    Co = dF.shape[1]
    _chk(dF, f32, "dF", (B, Co, H, W))
    _chk(Wp, f32, "Wp", (Co, Cc))
    split = Ci is not None and Ci != Cc
    Ci = Cc if not split else int(Ci)
    gu = torch.empty(B, H, W, Ci, device=t.device, dtype=bf16)
    gcs = torch.empty(B, H, W, Cc - Ci, device=t.device, dtype=bf16) if split else None
    _lib.call("edm_lowrank_gcat_add", _p(dF), _p(Wp), float(sa), _p(t), _p(gu), _p(gcs), B, H * W, Cc, Ci, Co, _stream())
    return gu, gcs


def nchw_to_nhwc_bf16(x):
    _chk(x, f32, "x")
    B, C, H, W = x.shape
    y = torch.empty(B, H, W, C, device=x.device, dtype=bf16)
    _lib.call("edm_nchw_to_nhwc_bf16", _p(x), _p(y), B, C, H * W, _stream())
    return y


def nhwc_bf16_to_nchw(x):
    B, H, W, C = _nhwc(x, "x")
    y = torch.empty(B, C, H, W, device=x.device, dtype=f32)
    _lib.call("edm_nhwc_bf16_to_nchw", _p(x), _p(y), B, C, H * W, _stream())
    return y


# ------------------------------------------------------------------ convolution
# 0 = pick per shape (default), 1 = register-staged 128x128 kernel, 2 = LDS-DMA 256x128 kernel,
# 5 = small-map split-K kernel, 6 = static-schedule 3x3 kernel (tests force each generation through this variable)
IGEMM_VERSION = int(os.environ.get("EDM_IGEMM", "0"))


# kernel ids of edm_conv_igemm_o / edm_conv_plan (include/tinyedm_hip.h)
_KERNEL_ID = {"edm_conv_igemm": 1, "edm_conv_igemm_v2": 2, "edm_conv_igemm_s": 5, "edm_conv_igemm_v6": 6}
_ENTRY = {kid: entry for entry, kid in _KERNEL_ID.items()}


@functools.lru_cache(maxsize=None)
def _conv_plan(B, H, W, Cin, Cout, taps, force):
    """edm_conv_plan: the kernel the library runs this shape on (id in the low byte, tile width of kernel 6 in the next).
    Asked once per shape and generation, and not through _lib.call: a host query is no launch (_lib.N_CALLS)."""
    return _lib.lib().edm_conv_plan(B, H, W, Cin, Cout, taps, force)


def _igemm_entry(npix, W, Cout, taps, Cin):
    """entry point of the kernel that runs npix = B * H * W pixels in rows of W (tests and tools ask by pixel count: the
    plan is asked for one image of npix // W rows; the launching functions below pass their real B and H)"""
    return _ENTRY[_conv_plan(1, npix // W, W, Cin, Cout, taps, IGEMM_VERSION) & 0xff]


def uses_s_kernel(B, H, W, Cin, Cout):
    """the default dispatch runs a 3x3 conv of this shape on k_conv3x3_s (the 8x8 layers' kernel) AND that kernel can take
    a fragment-major weight pack for it (networks._PrepPlan writes one for such layers)"""
    return (IGEMM_VERSION == 0 and Cout % 64 == 0 and Cin % 32 == 0
            and _conv_plan(B, H, W, Cin, Cout, 9, 0) & 0xff == 5)


def _wfrag(wp, plan, who):
    """1 when wp is a fragment-major pack (tagged by the plan that wrote it); such a pack is only valid on k_conv3x3_s"""
    if not getattr(wp, "_edm_frag", False):
        return 0
    if plan & 0xff != 5:
        raise ValueError(f"{who}: a fragment-major weight pack reached a shape that does not run on k_conv3x3_s ({_ENTRY[plan & 0xff]})")
    return 1


V46 = "_v6"     # profile-key suffix of the static-schedule 3x3 kernel (its 32x32x16 predecessor, "_v4", was retired in round 4)


def _conv_key(plan, taps=9, tail=""):
    """profile key naming the kernel that runs ("conv3x3_igemm_v6", "conv1x1_igemm", ...): _v6 = k_conv3x3_v6 with 512x128
    tiles, _v6s = the same kernel with 512x64 tiles (16x16 layers), _s = k_conv3x3_s (8x8 layers), _v2 = k_conv_igemm2"""
    suffix = {1: "", 2: "_v2", 5: "_s", 6: V46 if plan >> 8 == 128 else V46 + "s"}[plan & 0xff]
    return ("conv3x3_igemm" if taps == 9 else "conv1x1_igemm") + suffix + tail


def conv_igemm(x, wp, taps, residual=None, alpha=1.0, beta=0.0, out=None, silu_out=None, split=None):
    """Y = alpha*conv(x, wp) + beta*residual.  wp: bf16 (taps, Cout, Cin).
    Output descriptor (edm_conv_igemm_o; how the decoder's concat stops being a copy):
      out       a (B, H, W, Cout) VIEW with unit channel stride and a row stride >= Cout (the left column block of a wider
                NHWC buffer): the result is written there and `out` is returned;
      silu_out  a view with the same strides as `out`: also receives mp_silu(Y);
      split     (c, ya, yb): output channels < c go to ya (B, H, W, c), the others to yb (B, H, W, Cout - c), both
                contiguous; returns (ya, yb)."""
    B, H, W, Cin = _nhwc(x, "x")
    _chk(wp, bf16, "wp")
    if wp.dim() != 3 or wp.shape[0] != taps or wp.shape[2] != Cin:
        raise ValueError(f"conv_igemm: packed weight {tuple(wp.shape)} does not match taps={taps}, Cin={Cin}")
    Cout = wp.shape[1]
    if residual is not None:
        _chk(residual, bf16, "residual", (B, H, W, Cout))
    npix = B * H * W
    plan = _conv_plan(B, H, W, Cin, Cout, taps, IGEMM_VERSION)
    pname = _conv_key(plan, taps)
    nbytes = 2.0 * (npix * (Cin + Cout * ((2 if residual is not None else 1) + (1 if silu_out is not None else 0))) + wp.numel())
    wfrag = _wfrag(wp, plan, "conv_igemm")
    if out is None and silu_out is None and split is None and not wfrag:
        y = torch.empty(B, H, W, Cout, device=x.device, dtype=bf16)
        with _prof(pname, 2.0 * npix * Cin * Cout * taps, nbytes):
            _lib.call(_ENTRY[plan & 0xff], _p(x), _p(wp), _p(y), _p(residual), float(alpha), float(beta), B, H, W, Cin, Cout, taps, _stream())
        return y
    ld, ya, yb, ldb, c = 0, None, None, 0, 0
    if split is not None:
        if out is not None or silu_out is not None:
            raise ValueError("conv_igemm: split excludes out / silu_out")
        c, ya, yb = split
        _chk(ya, bf16, "split[1]", (B, H, W, c))
        _chk(yb, bf16, "split[2]", (B, H, W, Cout - c))
        if c % 8 or not (0 < c < Cout):
            raise ValueError("conv_igemm: split channel must be a multiple of 8 inside (0, Cout)")
        ld, ldb = c, Cout - c
    else:
        if out is None:
            out = torch.empty(B, H, W, Cout, device=x.device, dtype=bf16)
        ld = _row_view(out, B, H, W, Cout, "out")
        if silu_out is not None and _row_view(silu_out, B, H, W, Cout, "silu_out") != ld:
            raise ValueError("conv_igemm: out and silu_out must have the same row stride")
        ya = out
    with _prof(pname, 2.0 * npix * Cin * Cout * taps, nbytes):
        _lib.call("edm_conv_igemm_o", _p(x), _p(wp), _p(ya), ld, _p(silu_out), _p(yb), ldb, c, _p(residual), float(alpha),
                  float(beta), B, H, W, Cin, Cout, taps, plan & 0xff, wfrag, _stream())
    return (ya, yb) if split is not None else out


FOLD_PROJ = os.environ.get("EDM_FOLD_PROJ", "1") != "0"


def conv3x3_fold_supported(xshape, Cout, C2):
    """the shape (B, H, W, Cin) -> Cout of a decoder block's second 3x3 conv lets its skip projection (C2 -> Cout) ride along
    (conv3x3_fold)"""
    B, H, W, Cin = xshape
    return bool(FOLD_PROJ and IGEMM_VERSION == 0 and _lib.call("edm_conv3x3_fold_supported", B, H, W, Cin, Cout, C2))


def conv3x3_fold(x, wp, x2, w2p, alpha3, alpha1, out=None, silu_out=None):
    """Y = alpha3 * conv3x3(x, wp) + alpha1 * conv1x1(x2, w2p) in one launch (edm_conv3x3_fold): wp (9, Cout, Cin), x2
    (B, H, W, C2) contiguous, w2p (1, Cout, C2).  out / silu_out: the output descriptor of conv_igemm."""
    B, H, W, Cin = _nhwc(x, "x")
    _chk(wp, bf16, "wp")
    _chk(w2p, bf16, "w2p")
    B2, H2, W2, C2 = _nhwc(x2, "x2")
    Cout = wp.shape[1]
    if wp.dim() != 3 or wp.shape[0] != 9 or wp.shape[2] != Cin or tuple(w2p.shape) != (1, Cout, C2) or (B2, H2, W2) != (B, H, W):
        raise ValueError(f"conv3x3_fold: operands do not match (x {tuple(x.shape)}, wp {tuple(wp.shape)}, x2 {tuple(x2.shape)}, "
                         f"w2p {tuple(w2p.shape)})")
    if getattr(wp, "_edm_frag", False):
        raise ValueError("conv3x3_fold: a fragment-major weight pack belongs to k_conv3x3_s")
    if out is None:
        out = torch.empty(B, H, W, Cout, device=x.device, dtype=bf16)
    ld = _row_view(out, B, H, W, Cout, "out")
    if silu_out is not None and _row_view(silu_out, B, H, W, Cout, "silu_out") != ld:
        raise ValueError("conv3x3_fold: out and silu_out must have the same row stride")
    npix = B * H * W
    with _prof(_conv_key(_conv_plan(B, H, W, Cin, Cout, 9, 6), tail="_fold"), 2.0 * npix * Cout * (9 * Cin + C2),
               2.0 * (npix * (Cin + C2 + Cout * (2 if silu_out is not None else 1)) + wp.numel() + w2p.numel())):
        _lib.call("edm_conv3x3_fold", _p(x), _p(wp), _p(x2), C2, _p(w2p), C2, _p(out), ld, _p(silu_out), float(alpha3),
                  float(alpha1), B, H, W, Cin, Cout, _stream())
    return out


def _row_view(t, B, H, W, C, name):
    """row stride (elements) of a (B, H, W, C) bf16 view whose pixels are rows of one flat [B*H*W][ld] buffer"""
    if t.dtype != bf16 or not t.is_cuda or tuple(t.shape) != (B, H, W, C):
        raise ValueError(f"{name}: expected a cuda bf16 tensor of shape {(B, H, W, C)}, got {t.dtype} {tuple(t.shape)}")
    sb, sh, sw, sc = t.stride()
    if sc != 1 or sw < C or sw % 8 or sh != W * sw or sb != H * sh or (t.data_ptr() % 16):
        raise ValueError(f"{name}: strides {t.stride()} are not those of a column block of an NHWC buffer")
    return sw


FUSE_MOD = os.environ.get("EDM_FUSE_MOD", "1") != "0"


def conv3x3_mod(x, wp, lin, gain, pdrop, seed, sub, step, want_u=True, dyn=None, mark_dropped=False):
    """First 3x3 conv of a block with the modulation epilogue fused: returns (u, a2) with u = conv(x) (None when
    want_u is False) and a2 = dropout(mp_silu(u*(lin*gain+1))) -- same values as conv_igemm + mod_silu_drop_fwd.
    mark_dropped: the elements of u that the dropout removed come back as NaN (their value is never needed again);
    conv3x3_modbwd(u_marked=True) and mod_silu_drop_bwd read the mask from there."""
    B, H, W, Cin = _nhwc(x, "x")
    _chk(wp, bf16, "wp")
    if wp.dim() != 3 or wp.shape[0] != 9 or wp.shape[2] != Cin:
        raise ValueError(f"conv3x3_mod: pack shape {tuple(wp.shape)} does not match taps=9, Cin={Cin}")
    Cout = wp.shape[1]
    ls = _lin_view(lin, B, Cout, "lin")
    _chk(gain, f32, "gain")
    u = torch.empty(B, H, W, Cout, device=x.device, dtype=bf16) if want_u else None
    a2 = torch.empty(B, H, W, Cout, device=x.device, dtype=bf16)
    npix = B * H * W
    plan = _conv_plan(B, H, W, Cin, Cout, 9, 0)      # (the fused entry points launch from the automatic plan)
    with _prof(_conv_key(plan), 2.0 * npix * Cin * Cout * 9, 2.0 * (npix * (Cin + Cout * (2 if want_u else 1)) + wp.numel())):
        _lib.call("edm_conv3x3_mod", _p(x), _p(wp), _p(u), _p(a2), _p(lin), ls, _p(gain), float(pdrop), int(seed),
                  int(sub), int(step), int(bool(mark_dropped)), B, H, W, Cin, Cout, _dyn(dyn), _wfrag(wp, plan, "conv3x3_mod"),
                  _stream())
    return u, a2


def conv3x3_modbwd(gout, wd, alpha, r1, lin, gain, pdrop, seed, sub, step, glin_out=None, ggain_out=None, dyn=None,
                   gm_out=None, u_marked=False):
    """dgrad of a block's second 3x3 conv with the modulation backward in its epilogue: returns (gr1, glin, ggain),
    the values conv_igemm(gout, wd, 9, alpha=alpha) followed by mod_silu_drop_bwd would give (H*W % 32 == 0).
    gm_out: a zero-filled (B, Cout) fp32 view with unit column stride (a column slice of a buffer shared by all blocks):
    the raw modulation gradient is accumulated there and NOT finished -- returns (gr1, None, None); one
    mod_finish_multi over the shared buffer turns it into glin / ggain for every block.
    u_marked: r1 comes from conv3x3_mod(mark_dropped=True) with the same pdrop: dropped <=> NaN, no Philox stream is
    regenerated."""
    B, H, W, Cin = _nhwc(gout, "gout")
    _chk(wd, bf16, "wd")
    if wd.dim() != 3 or wd.shape[0] != 9 or wd.shape[2] != Cin:
        raise ValueError(f"conv3x3_modbwd: pack shape {tuple(wd.shape)} does not match taps=9, Cin={Cin}")
    Cout = wd.shape[1]
    _chk(r1, bf16, "r1", (B, H, W, Cout))
    if (H * W) % 32:
        raise ValueError("conv3x3_modbwd: H*W must be a multiple of 32")
    ls = _lin_view(lin, B, Cout, "lin")
    _chk(gain, f32, "gain")
    gr = torch.empty_like(r1)
    if gm_out is not None:
        gms = _lin_view(gm_out, B, Cout, "gm_out")
        gm = gm_out
    else:
        gms = 0
        gm = zeros_f32((B, Cout), r1.device)
        glin = torch.empty(B, Cout, device=r1.device, dtype=f32) if glin_out is None else glin_out
        gs = _lin_view(glin, B, Cout, "glin")
        ggain = zeros_f32((), r1.device) if ggain_out is None else _chk(ggain_out, f32, "ggain_out", ())
    npix = B * H * W
    plan = _conv_plan(B, H, W, Cin, Cout, 9, 0)      # (the fused entry points launch from the automatic plan)
    with _prof(_conv_key(plan, tail="_modbwd"), 2.0 * npix * Cin * Cout * 9, 2.0 * (npix * (Cin + 2 * Cout) + wd.numel())):
        _lib.call("edm_conv3x3_modbwd", _p(gout), _p(wd), float(alpha), _p(r1), _p(lin), ls, _p(gain), _p(gr), _p(gm), gms,
                  float(pdrop), int(seed), int(sub), int(step), int(bool(u_marked)), B, H, W, Cin, Cout, _dyn(dyn),
                  _wfrag(wd, plan, "conv3x3_modbwd"), _stream())
    if gm_out is not None:
        return gr, None, None
    _lib.call("edm_mod_finish", _p(gm), _p(lin), ls, _p(gain), _p(glin), gs, _p(ggain), B, Cout, _stream())
    return gr, glin, ggain


def mod_finish_multi(gm_all, lin_all, glin_all, items, n_items):
    """items: uint8 device tensor of n_items 24-byte records {gain ptr, ggain ptr, col0, C} (csrc/elementwise.hip
    ModFinItem): glin_all[:, col0:col0+C] += gm_all * gain, ggain += sum gm_all * lin_all, for every block at once."""
    _chk(gm_all, f32, "gm_all")
    _chk(lin_all, f32, "lin_all", gm_all.shape)
    _chk(glin_all, f32, "glin_all", gm_all.shape)
    _chk(items, torch.uint8, "items")
    if gm_all.dim() != 2 or items.numel() != 24 * n_items:
        raise ValueError("mod_finish_multi: bad buffers")
    _lib.call("edm_mod_finish_multi", _p(gm_all), _p(lin_all), _p(glin_all), gm_all.shape[1], _p(items), int(n_items),
              gm_all.shape[0], _stream())


def conv3x3_silubwd(g, wd, xpre, gextra=None, extra_scale=1.0):
    """dgrad of a block's first 3x3 conv with the mp_silu backward in its epilogue:
    mp_silu'(xpre) * conv_igemm(g, wd, 9) + extra_scale * gextra  (== conv_igemm followed by silu_bwd)."""
    B, H, W, Cin = _nhwc(g, "g")
    _chk(wd, bf16, "wd")
    if wd.dim() != 3 or wd.shape[0] != 9 or wd.shape[2] != Cin:
        raise ValueError(f"conv3x3_silubwd: pack shape {tuple(wd.shape)} does not match taps=9, Cin={Cin}")
    Cout = wd.shape[1]
    _chk(xpre, bf16, "xpre", (B, H, W, Cout))
    if gextra is not None:
        _chk(gextra, bf16, "gextra", xpre.shape)
    gx = torch.empty_like(xpre)
    npix = B * H * W
    plan = _conv_plan(B, H, W, Cin, Cout, 9, 0)      # (the fused entry points launch from the automatic plan)
    with _prof(_conv_key(plan, tail="_silubwd"), 2.0 * npix * Cin * Cout * 9,
               2.0 * (npix * (Cin + Cout * (3 if gextra is not None else 2)) + wd.numel())):
        _lib.call("edm_conv3x3_silubwd", _p(g), _p(wd), _p(xpre), _p(gextra), float(extra_scale), _p(gx), B, H, W, Cin,
                  Cout, _wfrag(wd, plan, "conv3x3_silubwd"), _stream())
    return gx


WGRAD_1X1 = os.environ.get("EDM_WGRAD_1X1", "1") != "0"
WGRAD_VERSION = 2       # (generation 1, the register-staged kernel, was retired in round 6; the name stays for the tests' asserts)


def conv_wgrad(x, dy, taps):
    """fp32 split-K slabs (S, taps, Cout, Cin) of dW in packed order."""
    B, H, W, Cin = _nhwc(x, "x")
    Bd, Hd, Wd, Cout = _nhwc(dy, "dy")
    if (Bd, Hd, Wd) != (B, H, W):
        raise ValueError("conv_wgrad: x/dy spatial mismatch")
    npix = B * H * W
    if taps == 1 and WGRAD_1X1 and Cin % 32 == 0 and Cout % 32 == 0:
        # dedicated 1x1 kernel: 256x128-output tiles (the 64x64 tiles below are L2->LDS bound on 1x1 layers)
        S = _lib.call("edm_conv_wgrad_1x1_nsplit", npix, Cin, Cout)
        slabs = torch.empty(S, 1, Cout, Cin, device=x.device, dtype=f32)
        with _prof("conv1x1_wgrad", 2.0 * npix * Cin * Cout, 2.0 * npix * (Cin + Cout) + 4.0 * slabs.numel()):
            _lib.call("edm_conv_wgrad_1x1", _p(x), _p(dy), _p(slabs), npix, Cin, Cout, S, _stream())
        return slabs
    S = _lib.call("edm_conv_wgrad_nsplit", B, H, W, Cin, Cout, taps)
    slabs = torch.empty(S, taps, Cout, Cin, device=x.device, dtype=f32)
    with _prof("conv3x3_wgrad" if taps == 9 else "conv1x1_wgrad", 2.0 * npix * Cin * Cout * taps,
               2.0 * npix * (Cin + Cout) + 4.0 * slabs.numel()):
        _lib.call("edm_conv_wgrad_v2", _p(x), _p(dy), _p(slabs), B, H, W, Cin, Cout, taps, S, _stream())
    return slabs


def wgrad1x1_group_supported(x, dy):
    return WGRAD_1X1 and x.shape[-1] % 32 == 0 and dy.shape[-1] % 32 == 0


def conv_wgrad_1x1_group(pairs):
    """pairs: sequence (<= 16) of (x, dy) NHWC bf16 tensors of 1x1 layers -> list of their fp32 split-K slabs
    (S, 1, Cout, Cin), all produced by ONE launch (csrc/conv_wgrad1x1.hip k_wgrad1x1_group)."""
    n = len(pairs)
    if not 0 < n <= 16:
        raise ValueError("conv_wgrad_1x1_group: 1..16 layers per group")
    arr = (_lib.WGrad1Item * n)()
    out = []
    flops = nbytes = 0.0
    for k, (x, dy) in enumerate(pairs):
        B, H, W, Cin = _nhwc(x, "x")
        Bd, Hd, Wd, Cout = _nhwc(dy, "dy")
        if (Bd, Hd, Wd) != (B, H, W) or Cin % 32 or Cout % 32:
            raise ValueError("conv_wgrad_1x1_group: x/dy mismatch or channels not multiples of 32")
        npix = B * H * W
        S = _lib.call("edm_conv_wgrad_1x1_nsplit_grouped", npix, Cin, Cout)
        slabs = torch.empty(S, 1, Cout, Cin, device=x.device, dtype=f32)
        arr[k] = _lib.WGrad1Item(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), npix, Cin, Cout, S, 0)
        out.append(slabs)
        flops += 2.0 * npix * Cin * Cout
        nbytes += 2.0 * npix * (Cin + Cout) + 4.0 * slabs.numel()
    th, td, defer, release = _tables.take(pairs[0][0].device)
    with _prof("conv1x1_wgrad", flops, nbytes):
        _lib.call("edm_conv_wgrad_1x1_group", ctypes.byref(arr), n, ctypes.c_void_p(th), ctypes.c_void_p(td), defer, _stream())
    release()
    return out


W3_MAX_LAYERS = 48      # csrc/conv_wgrad3.hip MAXL (edm_wgrad3_max_layers; checked by tests/test_host_cpu.py)


def wgrad3_supported(x, dy, I):
    """shapes the grouped 3x3 weight-gradient path (csrc/conv_wgrad3.hip) covers"""
    B, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    return Cin % 32 == 0 and Cout % 32 == 0 and W <= 126 and I * 9 * 4 <= 64 * 1024 and B * (H + 1) * (W + 1) < (1 << 30)


def wgrad3_plan_ksplit(shapes):
    """K shares per tile that edm_wgrad3_group's plan gives each layer of a group (diagnostics, host logic only: no
    launch, no device memory).  shapes: sequence of (B, H, W, Cin, Cout)."""
    n = len(shapes)
    arr = (_lib.WGrad3Item * n)()
    for k, (B, H, W, Cin, Cout) in enumerate(shapes):
        arr[k] = _lib.WGrad3Item(1, 1, 1, 1, None, B, H, W, Cin, Cout, Cin, 1.0, 0)     # (pointers only checked for NULL)
    out = (ctypes.c_int * n)()
    _lib.call("edm_wgrad3_plan_ksplit", ctypes.byref(arr), n, out)
    return list(out)


def wgrad3_group(items):
    """Weight gradients of up to W3_MAX_LAYERS (48) 3x3 conv layers in ONE stream-K launch + ONE finish launch.
    items: sequence of (x, dy, w, grad, perm, scale, accumulate) with x (B,H,W,Cin) / dy (B,H,W,Cout) NHWC bf16,
    w the fp32 master weight (Cout, I, 3, 3) with I <= Cin, grad an fp32 tensor like w that receives (accumulate=0)
    or accumulates (1) the projected gradient, perm the optional packed-row permutation (int32)."""
    arr, n, flops, nbytes = _wgrad3_items(items)
    return _wgrad3_launch(items, arr, n, flops, nbytes, "edm_wgrad3_group")


def _wgrad3_items(items):
    """the host descriptor array of a group (WGrad3Item per layer) after the shape checks, with its flop / byte counts"""
    n = len(items)
    if not 0 < n <= W3_MAX_LAYERS:
        raise ValueError(f"wgrad3_group: 1..{W3_MAX_LAYERS} layers per group")
    arr = (_lib.WGrad3Item * n)()
    flops = nbytes = 0.0
    halo = None
    for k, (x, dy, w, grad, perm, scale, accumulate) in enumerate(items):
        B, H, W, Cin = _nhwc(x, "x")
        Bd, Hd, Wd, Cout = _nhwc(dy, "dy")
        if (Bd, Hd, Wd) != (B, H, W):
            raise ValueError("wgrad3_group: x/dy spatial mismatch")
        _chk(w, f32, "w")
        if w.dim() != 4 or w.shape[0] != Cout or tuple(w.shape[2:]) != (3, 3) or w.shape[1] > Cin:
            raise ValueError(f"wgrad3_group: weight {tuple(w.shape)} does not match Cout={Cout}, Cin={Cin}")
        _chk(grad, f32, "grad", w.shape)
        if not wgrad3_supported(x, dy, w.shape[1]):
            raise ValueError(f"wgrad3_group: unsupported shape x={tuple(x.shape)} dy={tuple(dy.shape)}")
        if perm is not None:
            _chk(perm, torch.int32, "perm", (Cout,))
        h = W + 2 > 64
        if halo is not None and h != halo:
            raise ValueError("wgrad3_group: layers of one group must be all W <= 62 or all W > 62")
        halo = h
        arr[k] = _lib.WGrad3Item(x.data_ptr(), dy.data_ptr(), w.data_ptr(), grad.data_ptr(),
                                 None if perm is None else perm.data_ptr(), B, H, W, Cin, Cout, w.shape[1], float(scale),
                                 int(bool(accumulate)))
        flops += 2.0 * B * H * W * Cin * Cout * 9
        nbytes += 2.0 * B * H * W * (Cin + Cout) + 4.0 * w.numel()
    return arr, n, flops, nbytes


def _wgrad3_launch(items, arr, n, flops, nbytes, entry, *extra):
    """workspace, launch table and (when profiling) the kernel-only events around `entry`, edm_wgrad3_group or its
    apply form; `extra` are the arguments the apply form takes between defer_upload and the stream"""
    nb = _lib.call("edm_wgrad3_workspace", ctypes.byref(arr), n)
    if nb <= 0:
        raise _lib.HipKernelError(f"edm_wgrad3_workspace failed: {_lib.lib().edm_last_error().decode()}")
    work = torch.empty(nb // 4, device=items[0][0].device, dtype=f32)
    th, td, defer, release = _tables.take(items[0][0].device)
    probe = None
    if PROFILE is not None:
        # the entry point uploads its launch table, runs k_wgrad3 AND k_wgrad3_finish: "conv3x3_wgrad" times the call,
        # "conv3x3_wgrad_kernel" the k_wgrad3 launch alone (events recorded inside the call: edm_wgrad3_probe) -- the figure
        # the rocprofv3 kernel traces show (888 us per call vs 813-831 us for the kernel)
        probe = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        for ev in probe:
            ev.record()             # (torch creates the hipEvent_t on the first record)
        _lib.call("edm_wgrad3_probe", ctypes.c_void_p(probe[0].cuda_event), ctypes.c_void_p(probe[1].cuda_event))
    with _prof("conv3x3_wgrad", flops, nbytes):
        _lib.call(entry, ctypes.byref(arr), n, _p(work), nb, ctypes.c_void_p(th), ctypes.c_void_p(td), defer, *extra,
                  _stream())
    if probe is not None:
        PROFILE.setdefault("conv3x3_wgrad_kernel", []).append((probe[0], probe[1], flops, nbytes))
    release()
    return work


def wgrad3_group_apply(items, theta, m, v, ema, dyn, b1, b2, eps):
    """wgrad3_group whose finish pass applies the Adam + EMA update (ops.adam_ema's expressions, g = projected gradient
    * grad_scale) to the weight rows it holds instead of writing their gradient: theta, m, v and ema rows are rewritten,
    the gradient arena is not touched for them.  Every `w` of items is a slice of the flat arena `theta`; m, v and ema
    (None: no EMA) are arenas laid out like theta, and lr / ema_beta / grad_scale / bias corrections come from the device
    record `dyn` (edm_step_params).  A layer whose rows (I * 9 floats) exceed the kernel's register prefetch (7168) keeps the plain finish into its `grad`
    (accumulate as given).  The health word of the device gets bit 0 on a non-finite gradient or weight.
    Returns one bool per layer: True = updated here, False = its gradient is in `grad`."""
    arr, n, flops, nbytes = _wgrad3_items(items)
    _chk(theta, f32, "theta")
    if dyn is None:
        raise ValueError("wgrad3_group_apply: the device step record `dyn` is required")
    for t, name in ((m, "m"), (v, "v"), (ema, "ema")):
        if t is not None:
            _chk(t, f32, name, theta.shape)
    if m is None or v is None:
        raise ValueError("wgrad3_group_apply: m and v arenas are required")
    opt = (_lib.WGrad3Opt * n)()
    base, total = theta.data_ptr(), theta.numel()
    for k, (_, _, w, *_rest) in enumerate(items):
        off = w.data_ptr() - base
        if off < 0 or off % 4 or off // 4 + w.numel() > total:
            raise ValueError(f"wgrad3_group_apply: weight {k} is not a slice of the parameter arena")
        opt[k] = _lib.WGrad3Opt(m.data_ptr() + off, v.data_ptr() + off, None if ema is None else ema.data_ptr() + off)
    fused = (ctypes.c_int * n)()
    _wgrad3_launch(items, arr, n, flops, nbytes, "edm_wgrad3_group_apply", ctypes.byref(opt), _p(dyn), float(b1),
                   float(b2), float(eps), _p(health(theta.device)), fused)
    return [bool(f) for f in fused]


# ------------------------------------------------------------------ weights
def weight_prep(w, taps, Ipad=None, want_fwd=True, want_dgrad=True, want_hat=False, perm=None, normalize_inplace=False):
    """w: fp32 master (O, I, k, k) or (O, I).  Returns (wp_fwd, wp_dgrad, w_hat)."""
    _chk(w, f32, "w")
    O = w.shape[0]
    I = w.shape[1]
    if w.numel() != O * I * taps:
        raise ValueError("weight_prep: taps does not match the weight shape")
    Ipad = I if Ipad is None else Ipad
    dev = w.device
    wf = torch.empty(taps, O, Ipad, device=dev, dtype=bf16) if want_fwd else None
    wd = torch.empty(taps, I, O, device=dev, dtype=bf16) if want_dgrad else None
    wh = torch.empty(O, I * taps, device=dev, dtype=f32) if want_hat else None
    if perm is not None:
        _chk(perm, torch.int32, "perm", (O,))
    _lib.call("edm_weight_prep", _p(w), O, I, taps, Ipad, _p(wf), _p(wd), _p(wh), _p(perm), int(normalize_inplace),
              _stream())
    return wf, wd, wh


def weight_prep_multi(desc, groups, lds_bytes, normalize_inplace):
    """desc: uint8 tensor of 64-byte PrepDesc records (see csrc/weights.hip), groups: int32 [n_groups, 2] of
    (record, first row); lds_bytes: the largest rb*I*taps*2 over the records."""
    _chk(desc, torch.uint8, "desc")
    _chk(groups, torch.int32, "groups")
    if desc.numel() % 64 or groups.dim() != 2 or groups.shape[1] != 2:
        raise ValueError("weight_prep_multi: bad descriptor / group tables")
    _lib.call("edm_weight_prep_multi", _p(desc), _p(groups), int(groups.shape[0]), int(lds_bytes),
              int(bool(normalize_inplace)), _stream())


def wgrad_finish(slabs, w, taps, I, perm=None, scale=1.0, out=None):
    """Reduce slabs (S, taps, O, Ipad) and project through the weight normalisation -> grad like w."""
    _chk(slabs, f32, "slabs")
    _chk(w, f32, "w")
    S, t_, O, Ipad = slabs.shape
    if t_ != taps or w.shape[0] != O or w.numel() != O * I * taps:
        raise ValueError("wgrad_finish: shape mismatch")
    accumulate = out is not None
    if out is None:
        out = torch.empty_like(w)
    else:
        _chk(out, f32, "out", w.shape)
    _lib.call("edm_wgrad_finish", _p(slabs), S, _p(w), _p(out), _p(perm), O, I, Ipad, taps, float(scale), int(accumulate),
              _stream())
    return out


def wgrad_finish_multi(items):
    """items: sequence of (slabs, w, grad, perm, taps, I, scale, accumulate): wgrad_finish for all of them, 40 per launch"""
    for c0 in range(0, len(items), 40):
        chunk = items[c0:c0 + 40]
        arr = (_lib.FinishItem * len(chunk))()
        for k, (slabs, w, grad, perm, taps, I, scale, accumulate) in enumerate(chunk):
            _chk(slabs, f32, "slabs")
            _chk(w, f32, "w")
            S, t_, O, Ipad = slabs.shape
            if t_ != taps or w.shape[0] != O or w.numel() != O * I * taps:
                raise ValueError("wgrad_finish_multi: shape mismatch")
            _chk(grad, f32, "grad", w.shape)
            if perm is not None:
                _chk(perm, torch.int32, "perm", (O,))
            arr[k] = _lib.FinishItem(slabs.data_ptr(), w.data_ptr(), grad.data_ptr(), None if perm is None else perm.data_ptr(),
                                     S, O, I, Ipad, taps, float(scale), int(bool(accumulate)))
        th, td, defer, release = _tables.take(chunk[0][0].device)
        _lib.call("edm_wgrad_finish_multi", ctypes.byref(arr), len(chunk), ctypes.c_void_p(th), ctypes.c_void_p(td), defer,
                  _stream())
        release()


# ------------------------------------------------------------------ attention
def attention_fwd(qkv, heads):
    """qkv (B,H,W,3C) bf16 with per-token channel order [head][q|k|v][d] -> y (B,H,W,C)."""
    B, H, W, C3 = _nhwc(qkv, "qkv")
    C = C3 // 3
    y = torch.empty(B, H, W, C, device=qkv.device, dtype=bf16)
    N = H * W
    with _prof("attention_fwd", 4.0 * B * N * N * C, 2.0 * B * N * 4 * C):
        _lib.call("edm_attention_fwd", _p(qkv), _p(y), B, N, C, heads, _stream())
    return y


def attention_bwd(qkv, y, gy, heads):
    B, H, W, C3 = _nhwc(qkv, "qkv")
    C = C3 // 3
    _chk(y, bf16, "y", (B, H, W, C))
    _chk(gy, bf16, "gy", (B, H, W, C))
    gqkv = torch.empty_like(qkv)
    N = H * W
    with _prof("attention_bwd", 14.0 * B * N * N * C, 2.0 * B * N * 8 * C):
        _lib.call("edm_attention_bwd", _p(qkv), _p(y), _p(gy), _p(gqkv), B, N, C, heads, _stream())
    return gqkv


def attention_long_supported(N, C, heads):
    """the tiled-softmax kernels (attention_long.hip) cover this shape: any N >= 1, head_dim 64 / 32 / 128 / 144 / 192"""
    return bool(_lib.call("edm_attention_long_supported", N, C, heads))


def attention_long_fwd(qkv, heads, want_stat=True):
    """attention_fwd for any number of tokens: qkv (B,H,W,3C) bf16, channel order [head][q|k|v][d] ->
    y (B,H,W,C) bf16, stat (B, heads, H*W) fp32 = the rows' log-sum-exp, or None (networks.py:194-202)"""
    B, H, W, C3 = _nhwc(qkv, "qkv")
    C = C3 // 3
    N = H * W
    y = torch.empty(B, H, W, C, device=qkv.device, dtype=bf16)
    stat = torch.empty(B, heads, N, device=qkv.device, dtype=f32) if want_stat else None
    with _prof("attention_long_fwd", 4.0 * B * N * N * C, 2.0 * B * N * 4 * C):
        _lib.call("edm_attention_long_fwd", _p(qkv), _p(y), _p(stat), B, N, C, heads, _stream())
    return y, stat


def attention_long_bwd(qkv, y, gy, stat, heads):
    """-> gqkv (B,H,W,3C) bf16; y, stat = attention_long_fwd's outputs"""
    B, H, W, C3 = _nhwc(qkv, "qkv")
    C = C3 // 3
    N = H * W
    _chk(y, bf16, "y", (B, H, W, C))
    _chk(gy, bf16, "gy", (B, H, W, C))
    _chk(stat, f32, "stat", (B, heads, N))
    gqkv = torch.empty_like(qkv)
    work = torch.empty(B, heads, N, device=qkv.device, dtype=f32)     # delta = <dO, y>: query-major kernel -> key-major kernel
    with _prof("attention_long_bwd", 14.0 * B * N * N * C, 2.0 * B * N * 8 * C):
        _lib.call("edm_attention_long_bwd", _p(qkv), _p(y), _p(gy), _p(stat), _p(gqkv), _p(work), B, N, C, heads, _stream())
    return gqkv


ATTN_FUSED = os.environ.get("EDM_ATTN_FUSED", "1") != "0"      # qkv projection inside the attention kernels (attention_fused.hip)
ATTN_HP = int(os.environ.get("EDM_ATTN_HP", "0"))               # heads per workgroup of the FORWARD (0 = the kernel's default;
                                                                # the backward always runs one head per workgroup)


def attention_qkv_supported(x, heads):
    """the fused kernels cover this shape (C = 256, 4 heads of 64, 33..256 tokens)"""
    B, H, W, C = x.shape
    return bool(ATTN_FUSED and _lib.call("edm_attention_qkv_supported", H * W, C, heads))


def attention_qkv_fwd(x, wf_qkv, heads, want_stat=True):
    """x (B,H,W,C) bf16, wf_qkv (1, 3C, C) bf16 forward pack of the qkv conv (rows [head][q|k|v][d]) ->
    y (B,H,W,C) bf16 = cosine attention of qkv_conv(x), stat (B, heads, H*W) fp32 or None (networks.py:193-202)"""
    B, H, W, C = _nhwc(x, "x")
    _chk(wf_qkv, bf16, "wf_qkv", (1, 3 * C, C))
    N = H * W
    y = torch.empty_like(x)
    stat = torch.empty(B, heads, N, device=x.device, dtype=f32) if want_stat else None
    with _prof("attention_qkv_fwd", 2.0 * B * N * C * 3 * C + 4.0 * B * N * N * C, 2.0 * B * N * 2 * C):
        _lib.call("edm_attention_qkv_fwd", _p(x), _p(wf_qkv), _p(y), _p(stat), B, N, C, heads, ATTN_HP, _stream())
    return y, stat


def attention_qkv_bwd(x, y, gout, stat, wf_qkv, wd_out, heads, alpha=1.0):
    """-> gqkv (B,H,W,3C) bf16 (packed channel order) = d loss / d qkv_conv(x); gout = d loss / d out_conv(y),
    wd_out (1, C, C) = the out conv's dgrad pack; dO = alpha * gout . W_out is formed inside the kernel"""
    B, H, W, C = _nhwc(x, "x")
    _chk(y, bf16, "y", x.shape)
    _chk(gout, bf16, "gout", x.shape)
    _chk(stat, f32, "stat", (B, heads, H * W))
    _chk(wf_qkv, bf16, "wf_qkv", (1, 3 * C, C))
    _chk(wd_out, bf16, "wd_out", (1, C, C))
    N = H * W
    gqkv = torch.empty(B, H, W, 3 * C, device=x.device, dtype=bf16)
    with _prof("attention_qkv_bwd", 2.0 * B * N * C * 4 * C + 10.0 * B * N * N * C, 2.0 * B * N * 6 * C):
        _lib.call("edm_attention_qkv_bwd", _p(x), _p(y), _p(gout), _p(stat), _p(wf_qkv), _p(wd_out), _p(gqkv), float(alpha),
                  B, N, C, heads, 0, _stream())
    return gqkv


# ------------------------------------------------------------------ fp32 linears / embedding
_LINEAR_GEMM = {"fwd": lambda M, N, K: (M, N, K), "dgrad": lambda M, N, K: (M, K, N), "wgrad": lambda M, N, K: (N, K, M)}


def linear_plan(op, M, N, K, accumulate=0):
    """(tile_rows, splits) of the GEMM that edm_linear_<op>(M, N, K, accumulate) launches (host logic only: no launch, no
    device memory).  tile_rows 32 / 64 = the 32x64 / 64x64 tile; splits > 1 = split-K over atomics."""
    gm, gn, gk = _LINEAR_GEMM[op](M, N, K)
    rows, splits = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("edm_linear_plan", gm, gn, gk, int(accumulate), ctypes.byref(rows), ctypes.byref(splits))
    return rows.value, splits.value


def linear_fwd(x, w):
    _chk(x, f32, "x")
    _chk(w, f32, "w")
    M, K = x.shape
    N = w.shape[0]
    if w.shape != (N, K):
        raise ValueError("linear_fwd: shape mismatch")
    y = torch.empty(M, N, device=x.device, dtype=f32)
    _lib.call("edm_linear_fwd", _p(x), _p(w), _p(y), M, N, K, _stream())
    return y


def linear_dgrad(dy, w):
    _chk(dy, f32, "dy")
    _chk(w, f32, "w")
    M, N = dy.shape
    K = w.shape[1]
    if w.shape[0] != N:
        raise ValueError("linear_dgrad: shape mismatch")
    # (a pre-zeroed piece of the scratch pool + accumulate: the split-K form of the GEMM adds its partial sums with atomics and
    # would otherwise clear dx with a memset node of its own in every captured step)
    dx = zeros_f32((M, K), dy.device)
    _lib.call("edm_linear_dgrad", _p(dy), _p(w), _p(dx), M, N, K, 1, _stream())
    return dx


def linear_wgrad(dy, x):
    _chk(dy, f32, "dy")
    _chk(x, f32, "x")
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError("linear_wgrad: shape mismatch")
    dw = torch.empty(N, K, device=dy.device, dtype=f32)
    _lib.call("edm_linear_wgrad", _p(dy), _p(x), _p(dw), M, N, K, 0, _stream())
    return dw


def fourier_fwd(sigma, freqs, phases, B):
    ss = _sigma_arg(sigma, B)
    _chk(freqs, f32, "freqs")
    _chk(phases, f32, "phases", freqs.shape)
    out = torch.empty(B, freqs.numel(), device=freqs.device, dtype=f32)
    _lib.call("edm_fourier_fwd", _p(sigma), ss, _p(freqs), _p(phases), _p(out), B, freqs.numel(), _stream())
    return out


def _labels_arg(labels, B):
    if labels is None:
        return None
    if not labels.is_cuda:
        raise RuntimeError("labels must be a CUDA/HIP tensor")
    labels = labels.flatten().to(torch.int64).contiguous()
    if labels.numel() != B:
        raise ValueError(f"labels must have {B} elements")
    return labels


def label_drop_threshold(p) -> int:
    """the drop threshold of edm_embed_combine_fwd: round(p * 2^32) in fp64, clamped to [0, 2^32] (p = 0 drops no sample,
    p = 1 every one)"""
    return min(max(int(round(float(p) * 4294967296.0)), 0), 1 << 32)


def embed_combine_fwd(emb_sigma, wcls_hat, labels, add_factor, *, drop_p=0.0, seed=0, step=0, dyn=None, drop=None):
    """-> (pre, out); with label dropout (drop_p > 0 or a given mask `drop`, B int32 / bool, nonzero = dropped; needs
    labels) -> (pre, out, mask): the B int32 mask the kernel used, drawn from (seed, step) or dyn unless given.  A dropped
    sample's row is the labels=None row."""
    _chk(emb_sigma, f32, "emb_sigma")
    B, E = emb_sigma.shape
    K = 0
    if labels is not None:
        _chk(wcls_hat, f32, "wcls_hat")
        K = wcls_hat.shape[1]
    thr = label_drop_threshold(drop_p)
    masked = thr > 0 or drop is not None
    if masked and labels is None:
        raise ValueError("embed_combine_fwd: label dropout needs labels")
    drop_in = None
    if drop is not None:
        if not drop.is_cuda or drop.numel() != B:
            raise ValueError(f"embed_combine_fwd: drop must be a device tensor of {B} elements")
        drop_in = drop.flatten().to(torch.int32).contiguous()
    mask = torch.empty(B, device=emb_sigma.device, dtype=torch.int32) if masked else None
    pre, out = torch.empty_like(emb_sigma), torch.empty_like(emb_sigma)
    _lib.call("edm_embed_combine_fwd", _p(emb_sigma), _p(wcls_hat), _p(labels), float(add_factor), K, _p(pre), _p(out), B,
              E, thr, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, _dyn(dyn), _p(drop_in), _p(mask), _stream())
    return (pre, out, mask) if masked else (pre, out)


def embed_combine_bwd(gout, pre, labels, add_factor, wcls_shape, *, drop=None):
    """drop (nullable): the int32 mask embed_combine_fwd returned"""
    _chk(gout, f32, "gout", pre.shape)
    B, E = pre.shape
    ges = torch.empty_like(pre)
    gw, K = None, 0
    if labels is not None:
        gw = zeros_f32(wcls_shape, pre.device)
        K = wcls_shape[1]
    if drop is not None:
        if labels is None:
            raise ValueError("embed_combine_bwd: label dropout needs labels")
        _chk(drop, torch.int32, "drop", (B,))
    _lib.call("edm_embed_combine_bwd", _p(gout), _p(pre), _p(labels), float(add_factor), K, _p(ges), _p(gw), B, E, _p(drop),
              _stream())
    return ges, gw


def aug_embed_fwd(emb_sigma, aug, w_hat):
    """emb_sigma (B,E) += aug (B,K) @ w_hat (E,K)^T, IN PLACE (returns emb_sigma): the augment-label conditioning of
    Embedding(augment_dim=K), added to the output of the sigma Linear before embed_combine_fwd.  An all-zero row of aug
    leaves its row of emb_sigma unchanged."""
    _chk(emb_sigma, f32, "emb_sigma")
    if emb_sigma.dim() != 2:
        raise ValueError("aug_embed_fwd: emb_sigma must be (B, E)")
    B, E = emb_sigma.shape
    _chk(aug, f32, "aug")
    if aug.dim() != 2 or aug.shape[0] != B:
        raise ValueError(f"aug_embed_fwd: aug must be ({B}, K), got {tuple(aug.shape)}")
    K = aug.shape[1]
    _chk(w_hat, f32, "w_hat", (E, K))
    _lib.call("edm_aug_embed_fwd", _p(emb_sigma), _p(aug), _p(w_hat), B, E, K, _stream())
    return emb_sigma


def aug_embed_wgrad(gemb_sigma, aug):
    """-> gw_hat (E,K) = gemb_sigma (B,E)^T @ aug (B,K), summed over b in ascending order (bit-reproducible)."""
    _chk(gemb_sigma, f32, "gemb_sigma")
    if gemb_sigma.dim() != 2:
        raise ValueError("aug_embed_wgrad: gemb_sigma must be (B, E)")
    B, E = gemb_sigma.shape
    _chk(aug, f32, "aug")
    if aug.dim() != 2 or aug.shape[0] != B:
        raise ValueError(f"aug_embed_wgrad: aug must be ({B}, K), got {tuple(aug.shape)}")
    K = aug.shape[1]
    gw = torch.empty(E, K, device=gemb_sigma.device, dtype=f32)
    _lib.call("edm_aug_embed_wgrad", _p(gemb_sigma), _p(aug), _p(gw), B, E, K, _stream())
    return gw


# ------------------------------------------------------------------ the training step (csrc/optim.hip)
def diffuse(clean, P_mean, P_std, seed, step, dyn=None):
    _chk(clean, f32, "clean")
    B = clean.shape[0]
    noisy = torch.empty_like(clean)
    sigma = torch.empty(B, device=clean.device, dtype=f32)
    _lib.call("edm_diffuse", _p(clean), _p(noisy), _p(sigma), float(P_mean), float(P_std), B, clean.numel() // B, int(seed),
              int(step), _dyn(dyn), _stream())
    return noisy, sigma


def diffuse_given(clean, eps, noise, P_mean, P_std):
    _chk(clean, f32, "clean")
    B = clean.shape[0]
    _chk(eps, f32, "eps", (B,))
    _chk(noise, f32, "noise", clean.shape)
    noisy = torch.empty_like(clean)
    sigma = torch.empty(B, device=clean.device, dtype=f32)
    _lib.call("edm_diffuse_given", _p(clean), _p(eps), _p(noise), _p(noisy), _p(sigma), float(P_mean), float(P_std), B,
              clean.numel() // B, _stream())
    return noisy, sigma


def weighted_mse(D, clean, sigma, sigma_data, weight=None, want_grad=True, acc_sum=None, acc_total=None):
    """acc_sum (fp32, 1 element) / acc_total (int64, 1 element): the metric's epoch state, accumulated in the same pass"""
    _chk(D, f32, "D")
    _chk(clean, f32, "clean", D.shape)
    B = D.shape[0]
    if weight is not None:
        _chk(weight, f32, "weight", (B,))
    else:
        _chk(sigma, f32, "sigma", (B,))
    loss = zeros_f32((), D.device)
    dD = torch.empty_like(D) if want_grad else None
    if acc_sum is not None:
        _chk(acc_sum, f32, "acc_sum")
        _chk(acc_total, torch.int64, "acc_total")
    _lib.call("edm_weighted_mse", _p(D), _p(clean), _p(sigma), _p(weight), float(sigma_data), _p(loss), _p(dD), B,
              D.numel() // B, _p(acc_sum), _p(acc_total), _stream())
    return loss, dD


def adam_ema(theta, grad, m, v, ema, lr, b1, b2, eps, step, ema_beta, grad_scale=1.0, dyn=None, zero_grad=False):
    for t, nme in ((theta, "theta"), (grad, "grad"), (m, "m"), (v, "v")):
        _chk(t, f32, nme)
        if t.numel() != theta.numel():
            raise ValueError("adam_ema: arena size mismatch")
    if ema is not None:
        _chk(ema, f32, "ema")
    _lib.call("edm_adam_ema", _p(theta), _p(grad), _p(m), _p(v), _p(ema), theta.numel(), float(lr), float(b1), float(b2),
              float(eps), int(step), float(ema_beta), float(grad_scale), _dyn(dyn), int(bool(zero_grad)),
              _p(health(theta.device)), _stream())


ADAM_RANGE_CHUNK = 1024         # csrc/optim.hip ADAM_CHUNK: elements per workgroup of k_adam_ema_ranges


def complement_ranges(excluded, n):
    """[0, n) minus the `excluded` (offset, numel) slices, as a list of (first element, length)"""
    ranges, pos = [], 0
    for off, cnt in sorted((int(o), int(c)) for o, c in excluded):
        if cnt <= 0:
            continue
        if off < pos or off + cnt > n:
            raise ValueError(f"complement_ranges: slice ({off}, {cnt}) overlaps another or leaves the arena of {n}")
        if off > pos:
            ranges.append((pos, off - pos))
        pos = off + cnt
    if pos < n:
        ranges.append((pos, n - pos))
    return ranges


def adam_ranges_table(excluded, n, device):
    """Device table that drives adam_ema_ranges over [0, n) minus the `excluded` (offset, numel) slices: (ranges, chunks)
    with ranges int64 [R][2] = (first element, length) and chunks int32 [C][2] = (range id, offset inside the range), one
    entry per ADAM_RANGE_CHUNK elements.  Allocates and uploads: build it once per set, outside any stream capture."""
    ranges = complement_ranges(excluded, n)
    chunks = [(r, o) for r, (_, length) in enumerate(ranges) for o in range(0, length, ADAM_RANGE_CHUNK)]
    rt = torch.tensor(ranges, dtype=torch.int64).reshape(-1, 2).to(device)
    ct = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(device)
    return rt, ct


def adam_ema_ranges(theta, grad, m, v, ema, ranges, chunks, lr, b1, b2, eps, step, ema_beta, grad_scale=1.0, dyn=None,
                    zero_grad=False):
    """adam_ema over the element ranges of an adam_ranges_table only; everything outside them is left as it is (an empty
    table launches nothing).  Same expressions, health bit and zero_grad behaviour as adam_ema on the covered elements."""
    for t in (grad, m, v) + ((ema,) if ema is not None else ()):
        if t.numel() != theta.numel():
            raise ValueError("adam_ema_ranges: arena size mismatch")
    _chk(ranges, torch.int64, "ranges")
    _chk(chunks, torch.int32, "chunks")
    if ranges.dim() != 2 or ranges.shape[1] != 2 or chunks.dim() != 2 or chunks.shape[1] != 2:
        raise ValueError("adam_ema_ranges: ranges is int64 [R][2], chunks int32 [C][2]")
    _lib.call("edm_adam_ema_ranges", _p(theta), _p(grad), _p(m), _p(v), _p(ema), theta.numel(), _p(ranges),
              ranges.shape[0], _p(chunks), chunks.shape[0], float(lr), float(b1), float(b2), float(eps), int(step),
              float(ema_beta), float(grad_scale), _p(dyn), int(bool(zero_grad)), _p(health(theta.device)), _stream())


PHEMA_MAX_PROFILES = 4          # edm_adam_ema_phema: K
PHEMA_MAX_LENGTHS = 8           # edm_phema_accumulate: L


def adam_ema_phema(theta, grad, m, v, ema, profiles, betas, lr, b1, b2, eps, step, ema_beta, grad_scale=1.0, dyn=None,
                   zero_grad=False):
    """adam_ema plus the post-hoc EMA profiles: every tensor of `profiles` (1..4 fp32 arenas of theta's size) gets
    p = beta_k * p + (1 - beta_k) * theta_new in the same pass, beta_k read on the device from `betas` (K fp32)."""
    for t, nme in ((theta, "theta"), (grad, "grad"), (m, "m"), (v, "v")):
        _chk(t, f32, nme)
        if t.numel() != theta.numel():
            raise ValueError("adam_ema_phema: arena size mismatch")
    if ema is not None:
        _chk(ema, f32, "ema")
        if ema.numel() != theta.numel():
            raise ValueError("adam_ema_phema: arena size mismatch")
    profiles = list(profiles)
    K = len(profiles)
    if not 1 <= K <= PHEMA_MAX_PROFILES:
        raise ValueError(f"adam_ema_phema: 1 to {PHEMA_MAX_PROFILES} profiles, got {K}")
    for k, p in enumerate(profiles):
        _chk(p, f32, f"profiles[{k}]")
        if p.numel() != theta.numel() or p.device != theta.device:
            raise ValueError(f"adam_ema_phema: profiles[{k}] must be an arena of {theta.numel()} floats on {theta.device}")
    _chk(betas, f32, "betas", (K,))
    if betas.device != theta.device:
        raise ValueError(f"adam_ema_phema: betas must live on {theta.device}")
    ptrs = (ctypes.c_void_p * K)(*[p.data_ptr() for p in profiles])
    _lib.call("edm_adam_ema_phema", _p(theta), _p(grad), _p(m), _p(v), _p(ema), ptrs, K, _p(betas), theta.numel(),
              float(lr), float(b1), float(b2), float(eps), int(step), float(ema_beta), float(grad_scale), _dyn(dyn),
              int(bool(zero_grad)), _p(health(theta.device)), _stream())


# ---- guarded optimizer step (csrc/grad_guard.hip)
GUARD_BLOCK = 1024              # csrc/grad_guard.hip GUARD_BLOCK: elements per wave-level partial sum, counted from a tensor's start
GUARD_CHUNK = 4096              # default elements per workgroup of k_grad_guard_chunks: a table parameter (a multiple of
                                # GUARD_BLOCK) that moves work between workgroups, never a bit of the result
# edm_grad_guard_record (include/tinyedm_hip.h, csrc/common.h GuardRecord): 64 bytes
GUARD_RECORD = np.dtype([("coef", "<f4"), ("skip", "<u4"), ("norm", "<f4"), ("clip_value", "<f4"), ("sumsq", "<f8"),
                         ("steps", "<u8"), ("skipped", "<u8"), ("clipped", "<u8"), ("consecutive_skips", "<u4"),
                         ("pad", "<u4", (3,))])
assert GUARD_RECORD.itemsize == 64


class GuardTable(NamedTuple):
    """device tables and scratch of grad_guard over one arena layout (grad_guard_table)"""
    chunks: torch.Tensor        # int64 [C][3] = (tensor id, first element, length)
    tensors: torch.Tensor       # int32 [P][4] = (first chunk, number of chunks, first block, number of blocks)
    part: torch.Tensor          # float64 [NB]: block partials (scratch)
    flags: torch.Tensor         # int32 [NB + P]: non-finite flags of the blocks, then of the tensors (scratch)
    n: int                      # elements of the arena the table was built for


def grad_guard_chunks(offsets, numels, n, chunk=GUARD_CHUNK):
    """Host side of grad_guard_table: (chunks int64 [C][3], tensors int32 [P][4]) for parameter tensors at `offsets` with
    `numels` elements in an arena of n.  Tensor p is tiled exactly by consecutive chunks of at most `chunk` elements (a
    multiple of GUARD_BLOCK); no chunk straddles two tensors and none covers the padding between them.  tensors[p] also
    names the tensor's run of GUARD_BLOCK-element blocks in the partial-sum scratch.  Overlapping or outlying slices are
    refused (as by adam_ranges_table)."""
    offsets, numels, n, chunk = [int(o) for o in offsets], [int(c) for c in numels], int(n), int(chunk)
    if len(offsets) != len(numels) or not offsets:
        raise ValueError("grad_guard_table: one offset per tensor, at least one tensor")
    if chunk < GUARD_BLOCK or chunk % GUARD_BLOCK:
        raise ValueError(f"grad_guard_table: the chunk length must be a positive multiple of {GUARD_BLOCK}, got {chunk}")
    if any(c < 0 for c in numels):
        raise ValueError("grad_guard_table: negative tensor size")
    complement_ranges(zip(offsets, numels), n)        # raises on a slice that overlaps another or leaves [0, n)
    if any(c > 0 and (o < 0 or o + c > n) for o, c in zip(offsets, numels)):
        raise ValueError(f"grad_guard_table: a slice leaves the arena of {n}")
    chunks, tensors, blocks = [], [], 0
    for p, (off, cnt) in enumerate(zip(offsets, numels)):
        first, nb = len(chunks), (cnt + GUARD_BLOCK - 1) // GUARD_BLOCK
        chunks.extend((p, off + o, min(chunk, cnt - o)) for o in range(0, cnt, chunk))
        tensors.append((first, len(chunks) - first, blocks, nb))
        blocks += nb
    if not chunks:
        raise ValueError("grad_guard_table: every tensor is empty")
    if blocks >= 2 ** 31 or len(chunks) >= 2 ** 31:
        raise ValueError("grad_guard_table: the arena has too many blocks for the int32 table")
    return np.asarray(chunks, dtype=np.int64).reshape(-1, 3), np.asarray(tensors, dtype=np.int32).reshape(-1, 4)


def grad_guard_table(offsets, numels, n, device, chunk=GUARD_CHUNK) -> GuardTable:
    """Device chunk table (and scratch) that drives grad_guard over the parameter tensors of an arena of n elements.
    Allocates and uploads: build it once per optimizer, outside any stream capture."""
    if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("grad_guard_table: the chunk table cannot be built under stream capture")
    ch, tn = grad_guard_chunks(offsets, numels, n, chunk)
    nb = int(tn[:, 3].sum())
    return GuardTable(torch.from_numpy(ch).to(device), torch.from_numpy(tn).to(device),
                      torch.zeros(nb, dtype=torch.float64, device=device),
                      torch.zeros(nb + tn.shape[0], dtype=torch.int32, device=device), int(n))


def guard_record(device) -> torch.Tensor:
    """a zeroed device edm_grad_guard_record (8 int64 words: 64 bytes, 8-byte aligned)"""
    return torch.zeros(8, dtype=torch.int64, device=device)


def read_guard_record(record) -> dict:
    """the fields of a device guard record as Python numbers (one D2H copy, which waits for the stream)"""
    r = np.frombuffer(record.cpu().numpy().tobytes(), dtype=GUARD_RECORD)[0]
    return {k: r[k].item() for k in GUARD_RECORD.names if k != "pad"}


def _guard_record_ptr(record):
    if (not isinstance(record, torch.Tensor) or not record.is_cuda or not record.is_contiguous()
            or record.numel() * record.element_size() < 64 or record.data_ptr() % 8):
        raise ValueError("record: expected a contiguous, 8-byte-aligned device buffer of >= 64 bytes (ops.guard_record)")
    return ctypes.c_void_p(record.data_ptr())


def _guard_limit(x, name):
    """None / inf: off"""
    x = float("inf") if x is None else float(x)
    if not x >= 0.0:
        raise ValueError(f"grad_guard: {name} must be >= 0 (None or inf: off), got {x}")
    return x


def grad_guard(grad, table: GuardTable, sumsq, record, grad_scale=1.0, dyn=None, max_norm=None, clip_value=None,
               skip_nonfinite=False, count=True):
    """One reduction over the gradient arena `grad` (fp32, any 4-byte-aligned view): sumsq[p] = sum (g * grad_scale)^2 of
    tensor p in fp64 and the device `record` (norm, clip coefficient, skip decision, counters) that adam_ema_guarded reads.
    Fixed summation order: bit-identical from run to run and for any chunk length of the table.  Nothing is read back;
    three launches on the current stream."""
    _chk(grad, f32, "grad")
    if grad.numel() != table.n:
        raise ValueError(f"grad_guard: the table was built for an arena of {table.n} elements, grad has {grad.numel()}")
    C, P, NB = table.chunks.shape[0], table.tensors.shape[0], table.part.shape[0]
    _chk(table.chunks, torch.int64, "chunks", (C, 3))
    _chk(table.tensors, torch.int32, "tensors", (P, 4))
    _chk(table.part, torch.float64, "part", (NB,))
    _chk(table.flags, torch.int32, "flags", (NB + P,))
    _chk(sumsq, torch.float64, "sumsq", (P,))
    for t in (table.chunks, table.tensors, table.part, table.flags, sumsq, record):
        if t.device != grad.device:
            raise ValueError(f"grad_guard: tables, sums and record must live on {grad.device}")
    _lib.call("edm_grad_guard", _p(grad), grad.numel(), _p(table.chunks), C, _p(table.tensors), P, NB, float(grad_scale),
              _dyn(dyn), _guard_limit(max_norm, "max_norm"), _guard_limit(clip_value, "clip_value"),
              int(bool(skip_nonfinite)), int(bool(count)), _p(table.part), _p(table.flags), _p(sumsq),
              _guard_record_ptr(record), _stream())


def adam_ema_guarded(theta, grad, m, v, ema, record, lr, b1, b2, eps, step, ema_beta, grad_scale=1.0, dyn=None,
                     zero_grad=False):
    """adam_ema behind a grad_guard `record` of the same stream: gradient scale grad_scale * coef, each scaled element
    limited to +-clip_value; a record with skip set leaves theta / m / v / ema bit for bit (grad is still cleared when
    zero_grad, the health word is not touched)."""
    for t, nme in ((theta, "theta"), (grad, "grad"), (m, "m"), (v, "v")):
        _chk(t, f32, nme)
        if t.numel() != theta.numel():
            raise ValueError("adam_ema_guarded: arena size mismatch")
    if ema is not None:
        _chk(ema, f32, "ema")
        if ema.numel() != theta.numel():
            raise ValueError("adam_ema_guarded: arena size mismatch")
    _lib.call("edm_adam_ema_guarded", _p(theta), _p(grad), _p(m), _p(v), _p(ema), theta.numel(), float(lr), float(b1),
              float(b2), float(eps), int(step), float(ema_beta), float(grad_scale), _dyn(dyn), int(bool(zero_grad)),
              _guard_record_ptr(record), _p(health(theta.device)), _stream())


def adam_ema_phema_guarded(theta, grad, m, v, ema, profiles, betas, record, lr, b1, b2, eps, step, ema_beta,
                           grad_scale=1.0, dyn=None, zero_grad=False):
    """adam_ema_phema behind a grad_guard `record` (see adam_ema_guarded); a skipped step leaves the profiles alone too."""
    for t, nme in ((theta, "theta"), (grad, "grad"), (m, "m"), (v, "v")):
        _chk(t, f32, nme)
        if t.numel() != theta.numel():
            raise ValueError("adam_ema_phema_guarded: arena size mismatch")
    if ema is not None:
        _chk(ema, f32, "ema")
        if ema.numel() != theta.numel():
            raise ValueError("adam_ema_phema_guarded: arena size mismatch")
    profiles = list(profiles)
    K = len(profiles)
    if not 1 <= K <= PHEMA_MAX_PROFILES:
        raise ValueError(f"adam_ema_phema_guarded: 1 to {PHEMA_MAX_PROFILES} profiles, got {K}")
    for k, p in enumerate(profiles):
        _chk(p, f32, f"profiles[{k}]")
        if p.numel() != theta.numel() or p.device != theta.device:
            raise ValueError(f"adam_ema_phema_guarded: profiles[{k}] must be an arena of {theta.numel()} floats on {theta.device}")
    _chk(betas, f32, "betas", (K,))
    if betas.device != theta.device:
        raise ValueError(f"adam_ema_phema_guarded: betas must live on {theta.device}")
    ptrs = (ctypes.c_void_p * K)(*[p.data_ptr() for p in profiles])
    _lib.call("edm_adam_ema_phema_guarded", _p(theta), _p(grad), _p(m), _p(v), _p(ema), ptrs, K, _p(betas), theta.numel(),
              float(lr), float(b1), float(b2), float(eps), int(step), float(ema_beta), float(grad_scale), _dyn(dyn),
              int(bool(zero_grad)), _guard_record_ptr(record), _p(health(theta.device)), _stream())


def phema_accumulate(acc, snap, weights):
    """acc[l] += weights[l] * snap for every row l of the fp64 accumulator acc [L, n] (L <= 8); snap: fp32, n elements"""
    _chk(acc, torch.float64, "acc")
    _chk(snap, f32, "snap")
    if acc.dim() != 2 or snap.numel() != acc.shape[1] or snap.device != acc.device:
        raise ValueError(f"phema_accumulate: acc [L, n] and snap [n] on one device, got {tuple(acc.shape)} and "
                         f"{tuple(snap.shape)}")
    L = acc.shape[0]
    w = [float(x) for x in weights]
    if len(w) != L or not 1 <= L <= PHEMA_MAX_LENGTHS:
        raise ValueError(f"phema_accumulate: 1 to {PHEMA_MAX_LENGTHS} weights, one per row of acc, got {len(w)} for {L} rows")
    if not all(math.isfinite(x) for x in w):
        raise ValueError("phema_accumulate: weights must be finite")
    _lib.call("edm_phema_accumulate", _p(acc), _p(snap), (ctypes.c_double * L)(*w), L, acc.shape[1], _stream())


def phema_finish(acc):
    """fp64 accumulator -> fp32 (round to nearest), same shape"""
    _chk(acc, torch.float64, "acc")
    out = torch.empty(acc.shape, device=acc.device, dtype=f32)
    if acc.numel():
        _lib.call("edm_phema_finish", _p(acc), _p(out), acc.numel(), _stream())
    return out


# ------------------------------------------------------------------ the updates of the samplers (csrc/solver_steps.hip)
def heun_euler(x, D, t0, t1):
    _chk(x, f32, "x")
    _chk(D, f32, "D", x.shape)
    dx, x1 = torch.empty_like(x), torch.empty_like(x)
    _lib.call("edm_heun_euler", _p(x), _p(D), float(t0), float(t1), _p(dx), _p(x1), x.numel(), _p(health(x.device)),
              _stream())
    return dx, x1


def heun_correct(x, dx, x1, D1, t0, t1):
    _chk(x, f32, "x")
    out = torch.empty_like(x)
    _lib.call("edm_heun_correct", _p(x), _p(dx), _p(x1), _p(D1), float(t0), float(t1), _p(out), x.numel(),
              _p(health(x.device)), _stream())
    return out


def _guidance_weight(w_dev, x):
    _chk(w_dev, f32, "w_dev")
    if w_dev.numel() != 1 or w_dev.device != x.device:
        raise ValueError(f"w_dev: expected a one-element fp32 tensor on {x.device}, got {tuple(w_dev.shape)} on "
                         f"{w_dev.device}")


def heun_euler_guided(x, Dm, Dg, w_dev, t0, t1):
    """heun_euler on D = Dg + w*(Dm - Dg), w read on the device from the one-element tensor w_dev"""
    _chk(x, f32, "x")
    _chk(Dm, f32, "Dm", x.shape)
    _chk(Dg, f32, "Dg", x.shape)
    _guidance_weight(w_dev, x)
    dx, x1 = torch.empty_like(x), torch.empty_like(x)
    _lib.call("edm_heun_euler_guided", _p(x), _p(Dm), _p(Dg), _p(w_dev), float(t0), float(t1), _p(dx), _p(x1),
              x.numel(), _p(health(x.device)), _stream())
    return dx, x1


def heun_correct_guided(x, dx, x1, Dm1, Dg1, w_dev, t0, t1):
    """heun_correct on D1 = Dg1 + w*(Dm1 - Dg1), w read on the device from the one-element tensor w_dev"""
    _chk(x, f32, "x")
    _chk(dx, f32, "dx", x.shape)
    _chk(x1, f32, "x1", x.shape)
    _chk(Dm1, f32, "Dm1", x.shape)
    _chk(Dg1, f32, "Dg1", x.shape)
    _guidance_weight(w_dev, x)
    out = torch.empty_like(x)
    _lib.call("edm_heun_correct_guided", _p(x), _p(dx), _p(x1), _p(Dm1), _p(Dg1), _p(w_dev), float(t0), float(t1),
              _p(out), x.numel(), _p(health(x.device)), _stream())
    return out


def churn_record(seed: int, solve_index: int, device=None, out=None):
    """The four-word device record edm_heun_churn reads its stream from: {seed_lo, seed_hi, solve_index, 0} as uint32,
    held in an int32 tensor.  Writes into `out` when given (one host->device copy), else allocates on `device`."""
    seed, solve_index = int(seed), int(solve_index)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"churn_record: seed must be in [0, 2**64), got {seed}")
    if not 0 <= solve_index < 1 << 32:
        raise ValueError(f"churn_record: solve_index must be in [0, 2**32), got {solve_index}")
    words = (seed & 0xFFFFFFFF, seed >> 32, solve_index, 0)
    host = torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32)   # (the uint32 bits)
    if out is None:
        return host.to(device)
    _churn_rec(out, out)
    out.copy_(host)
    return out


def _churn_rec(rec, x):
    _chk(rec, torch.int32, "rec")
    if rec.numel() != 4 or rec.device != x.device:
        raise ValueError(f"rec: expected a four-element int32 tensor on {x.device} (ops.churn_record), got "
                         f"{tuple(rec.shape)} on {rec.device}")


def heun_churn(x, c, rec, step):
    """x_hat = x + c*n with n ~ N(0, 1) drawn in the kernel (the churn of the stochastic sampler).  x: contiguous fp32
    [B, ...]; rec: the device record of ops.churn_record (seed, solve index); step: the solver step, part of the
    Philox counter.  The noise of sample b depends only on (seed, solve index, step, b, element)."""
    _chk(x, f32, "x")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"x: expected a non-empty [B, ...] tensor, got {tuple(x.shape)}")
    _churn_rec(rec, x)
    c, step = float(c), int(step)
    if not math.isfinite(c):
        raise ValueError(f"heun_churn: c must be finite, got {c}")
    if not 0 <= step < 1 << 31:
        raise ValueError(f"heun_churn: step must be in [0, 2**31), got {step}")
    B = x.shape[0]
    x_hat = torch.empty_like(x)
    _lib.call("edm_heun_churn", _p(x), c, _p(rec), step, B, x.numel() // B, _p(x_hat), _p(health(x.device)),
              _stream())
    return x_hat


def dpm_multistep(x, Dm, a, c0, c1=0.0, c2=0.0, Dg=None, w_dev=None, m1=None, m2=None, m_out=None):
    """One DPM-Solver++ multistep update: m = Dg + w*(Dm - Dg) (w read on the device from the one-element tensor
    w_dev) when Dg is given, else m = Dm; returns x_out = a*x + c0*m + c1*m1 + c2*m2 and writes m to m_out when given.
    m1 / m2: the previous steps' m (None drops the term, so its coefficient must be 0).  Every tensor fp32, contiguous,
    x's shape and device; m_out aliases no operand."""
    _chk(x, f32, "x")
    if x.numel() == 0:
        raise ValueError("x: expected a non-empty tensor")
    _chk(Dm, f32, "Dm", x.shape)
    if (Dg is None) != (w_dev is None):
        raise ValueError("dpm_multistep: Dg and w_dev go together (guided) or are both None")
    if Dg is not None:
        _chk(Dg, f32, "Dg", x.shape)
        _guidance_weight(w_dev, x)
    a, c0, c1, c2 = float(a), float(c0), float(c1), float(c2)
    if not all(math.isfinite(v) for v in (a, c0, c1, c2)):
        raise ValueError(f"dpm_multistep: coefficients must be finite, got {(a, c0, c1, c2)}")
    if m1 is None and m2 is not None:
        raise ValueError("dpm_multistep: m2 needs m1")
    for t, c, nme in ((m1, c1, "m1"), (m2, c2, "m2")):
        if t is None and c != 0.0:
            raise ValueError(f"dpm_multistep: {nme} is None but its coefficient is {c}")
    ins = [(t, nme) for t, nme in ((x, "x"), (Dm, "Dm"), (Dg, "Dg"), (m1, "m1"), (m2, "m2")) if t is not None]
    for t, nme in ins[1:] + ([(m_out, "m_out")] if m_out is not None else []):
        _chk(t, f32, nme, x.shape)
        if t.device != x.device:
            raise ValueError(f"{nme}: expected a tensor on {x.device}, got {t.device}")
    if m_out is not None and any(t.data_ptr() == m_out.data_ptr() for t, _ in ins):
        raise ValueError("m_out: must not alias an operand")
    x_out = torch.empty_like(x)
    _lib.call("edm_dpm_multistep", _p(x), _p(Dm), _p(Dg), _p(w_dev), _p(m1), _p(m2), a, c0, c1, c2, _p(x_out),
              _p(m_out), x.numel(), _p(health(x.device)), _stream())
    return x_out


def state_init(x0, t, image=None):
    """The state of a solve at noise level t: image + t*x0 (one fma), x0 the unit noise.  image=None: x0*t, bit for bit
    scale_f32(x0, t).  x0 / image: contiguous fp32 of one shape on one device; t finite and >= 0."""
    _chk(x0, f32, "x0")
    if x0.numel() == 0:
        raise ValueError("x0: expected a non-empty tensor")
    if image is not None:
        _chk(image, f32, "image", x0.shape)
        if image.device != x0.device:
            raise ValueError(f"image: expected a tensor on {x0.device}, got {image.device}")
    t = float(t)
    if not (math.isfinite(t) and t >= 0.0):
        raise ValueError(f"state_init: t must be finite and >= 0, got {t}")
    out = torch.empty_like(x0)
    _lib.call("edm_state_init", _p(image), _p(x0), t, _p(out), x0.numel(), _p(health(x0.device)), _stream())
    return out


INPAINT_MAX_STEPS = 1 << 16     # step < 2**16 keeps the blend's Philox tag apart from the churn's for every pair of steps


def inpaint_blend(x, image, mask, t, rec, step):
    """out = mask ? image + t*n : x with n ~ N(0, 1) drawn in the kernel (the replacement step of inpainting).  x, image:
    contiguous fp32 [B, C, ...]; mask: contiguous uint8 [mask_B, HW] with mask_B in {1, B} and HW the number of pixels,
    non-zero = known pixel, broadcast over the channels (and the batch when mask_B == 1); rec: the device record of
    ops.churn_record (seed, solve index); step: the solver step, part of the Philox counter.  The noise of sample b
    depends only on (seed, solve index, step, b, element) and is independent of heun_churn's.  t == 0 gives image itself
    on the mask."""
    _chk(x, f32, "x")
    if x.dim() < 3 or x.numel() == 0:
        raise ValueError(f"x: expected a non-empty [B, C, ...] tensor, got {tuple(x.shape)}")
    _chk(image, f32, "image", x.shape)
    _chk(mask, torch.uint8, "mask")
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    if mask.dim() != 2 or mask.shape[0] not in (1, B) or mask.shape[1] != HW:
        raise ValueError(f"mask: expected uint8 [1 or {B}, {HW}], got {tuple(mask.shape)}")
    for tt, nme in ((image, "image"), (mask, "mask")):
        if tt.device != x.device:
            raise ValueError(f"{nme}: expected a tensor on {x.device}, got {tt.device}")
    _churn_rec(rec, x)
    t, step = float(t), int(step)
    if not (math.isfinite(t) and t >= 0.0):
        raise ValueError(f"inpaint_blend: t must be finite and >= 0, got {t}")
    if not 0 <= step < INPAINT_MAX_STEPS:
        raise ValueError(f"inpaint_blend: step must be in [0, {INPAINT_MAX_STEPS}), got {step}")
    out = torch.empty_like(x)
    _lib.call("edm_inpaint_blend", _p(x), _p(image), _p(mask), t, _p(rec), step, B, C, HW, mask.shape[0], _p(out),
              _p(health(x.device)), _stream())
    return out


def scale_f32(x, s):
    _chk(x, f32, "x")
    y = torch.empty_like(x)
    _lib.call("edm_scale_f32", _p(x), float(s), _p(y), x.numel(), _stream())
    return y


# ------------------------------------------------------------------ zero-shot restoration (csrc/restore.hip)
RESTORE_SCALES = (1, 2, 4, 8)   # block sizes of the restoration operator (csrc/restore.hip)
RESTORE_MAX_GRAY_CHANNELS = 8


def check_degradation(scale, gray) -> None:
    """the operator settings that need no tensor: scale in RESTORE_SCALES, gray a bool, not the identity"""
    if isinstance(scale, bool) or not isinstance(scale, int) or scale not in RESTORE_SCALES:
        raise ValueError(f"degradation: scale must be one of {RESTORE_SCALES}, got {scale!r}")
    if not isinstance(gray, bool):
        raise ValueError(f"degradation: gray must be a bool, got {gray!r}")
    if scale == 1 and not gray:
        raise ValueError("degradation: scale == 1 without gray is the identity: nothing to restore")


def measurement_shape(x_shape, scale, gray) -> tuple:
    """the shape of y = A x for x of shape [B, C, H, W]; raises ValueError where A is not defined"""
    check_degradation(scale, gray)
    if len(x_shape) != 4 or any(int(v) < 1 for v in x_shape):
        raise ValueError(f"degradation: expected a non-empty [B, C, H, W] shape, got {tuple(x_shape)}")
    B, C, H, W = (int(v) for v in x_shape)
    if H % scale or W % scale:
        raise ValueError(f"degradation: H and W must be multiples of scale = {scale}, got {H} x {W}")
    if gray and C > RESTORE_MAX_GRAY_CHANNELS:
        raise ValueError(f"degradation: gray averages at most {RESTORE_MAX_GRAY_CHANNELS} channels, got {C}")
    return (B, 1 if gray else C, H // scale, W // scale)


def degrade(x, scale, gray):
    """y = A x: the mean of every scale x scale pixel block of x [B, C, H, W] (contiguous fp32), and with gray also over
    the channels: [B, 1 if gray else C, H/scale, W/scale].  Order-fixed sum (include/tinyedm_hip.h)."""
    _chk(x, f32, "x")
    shape = measurement_shape(x.shape, scale, gray)
    y = torch.empty(shape, device=x.device, dtype=f32)
    _lib.call("edm_degrade", _p(x), _p(y), *x.shape, scale, int(gray), _stream())
    return y


def project_denoised(Dm, y, scale, gray, Dg=None, w_dev=None, out=None):
    """D + A+ (y - A D): the projection of a denoiser output onto the images whose measurement is y (DDNM).  D = Dm, or
    with Dg and w_dev (the one-element device tensor of the guided updates) D = Dg + w*(Dm - Dg).  Dm / Dg / out:
    contiguous fp32 [B, C, H, W] on one device, y: contiguous fp32 of measurement_shape(Dm.shape, scale, gray); out
    (allocated when None) aliases no operand.  project_denoised(D, degrade(D)) == D and project_denoised(0, y) == A+ y
    bit for bit."""
    _chk(Dm, f32, "Dm")
    _chk(y, f32, "y", measurement_shape(Dm.shape, scale, gray))
    if (Dg is None) != (w_dev is None):
        raise ValueError("project_denoised: Dg and w_dev go together (guided) or are both None")
    if Dg is not None:
        _chk(Dg, f32, "Dg", Dm.shape)
        _guidance_weight(w_dev, Dm)
    if out is None:
        out = torch.empty_like(Dm)
    else:
        _chk(out, f32, "out", Dm.shape)
    ins = [(t, nme) for t, nme in ((Dm, "Dm"), (y, "y"), (Dg, "Dg")) if t is not None]
    for t, nme in ins[1:] + [(out, "out")]:
        if t.device != Dm.device:
            raise ValueError(f"{nme}: expected a tensor on {Dm.device}, got {t.device}")
    if any(t.data_ptr() == out.data_ptr() for t, _ in ins):
        raise ValueError("out: must not alias an operand")
    _lib.call("edm_project_denoised", _p(Dm), _p(Dg), _p(w_dev), _p(y), _p(out), *Dm.shape, scale, int(gray),
              _p(health(Dm.device)), _stream())
    return out


# ------------------------------------------------------------------ diffusion posterior sampling (csrc/restore.hip)
BLUR_MAX_RADIUS = 4


def degrade_adjoint(r, channels, scale, gray):
    """A^T r for the averaging A of degrade(): r (contiguous fp32, the measurement shape of a [B, channels, H, W] image) ->
    [B, channels, H, W], every value replicated to its block (and channels, gray) and divided by the block size"""
    _chk(r, f32, "r")
    if r.dim() != 4:
        raise ValueError(f"degrade_adjoint: expected a [B, C', h, w] measurement, got {tuple(r.shape)}")
    shape = (r.shape[0], int(channels), r.shape[2] * scale, r.shape[3] * scale)
    if tuple(r.shape) != measurement_shape(shape, scale, gray):
        raise ValueError(f"degrade_adjoint: r of shape {tuple(r.shape)} is no measurement of a {channels}-channel image")
    out = torch.empty(shape, device=r.device, dtype=f32)
    _lib.call("edm_degrade_adjoint", _p(r), _p(out), *shape, scale, int(gray), _stream())
    return out


def gaussian_taps(std, radius) -> tuple:
    """the 2*radius+1 normalised taps exp(-k^2 / (2 std^2)) / sum of a GaussianBlur, as fp32 values (host only)"""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= BLUR_MAX_RADIUS:
        raise ValueError(f"blur: radius must be an integer in [1, {BLUR_MAX_RADIUS}], got {radius!r}")
    std = float(std)
    if not (math.isfinite(std) and std > 0.0):
        raise ValueError(f"blur: std must be positive and finite, got {std}")
    raw = [math.exp(-(k * k) / (2.0 * std * std)) for k in range(-radius, radius + 1)]
    tot = sum(raw)
    return tuple(float(torch.tensor(v / tot, dtype=f32)) for v in raw)


def blur2d(x, taps):
    """y = K x: the separable zero-padded blur with the odd-length tap tuple `taps` on every H x W plane of x (contiguous
    fp32 [..., H, W]); order-fixed fma chains (include/tinyedm_hip.h)"""
    _chk(x, f32, "x")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"blur2d: expected a non-empty [..., H, W] tensor, got {tuple(x.shape)}")
    n = len(taps)
    if n % 2 == 0 or not 3 <= n <= 2 * BLUR_MAX_RADIUS + 1:
        raise ValueError(f"blur2d: 3, 5, 7 or 9 taps, got {n}")
    H, W = x.shape[-2:]
    y = torch.empty_like(x)
    arr = (ctypes.c_float * n)(*[float(t) for t in taps])
    _lib.call("edm_blur2d", _p(x), _p(y), ctypes.cast(arr, ctypes.c_void_p), n // 2, x.numel() // (H * W), H, W, _stream())
    return y


def dps_residual(y, AD):
    """(r, nrm): r = y - AD (contiguous fp32 [B, ...] of one shape) and nrm[b] = ||r_b||_2, an order-fixed reduction (the same
    bits on every run and for every B)"""
    _chk(y, f32, "y")
    _chk(AD, f32, "AD", y.shape)
    if y.dim() < 2 or y.numel() == 0:
        raise ValueError(f"dps_residual: expected a non-empty [B, ...] tensor, got {tuple(y.shape)}")
    if AD.device != y.device:
        raise ValueError(f"AD: expected a tensor on {y.device}, got {AD.device}")
    B = y.shape[0]
    r = torch.empty_like(y)
    nrm = torch.empty(B, device=y.device, dtype=f32)
    _lib.call("edm_dps_residual", _p(y), _p(AD), _p(r), _p(nrm), B, y.numel() // B, _stream())
    return r, nrm


def dps_update(x, g, nrm, scale):
    """x + (scale / nrm[b]) * g per sample (x where nrm[b] == 0 or scale == 0, bit for bit): contiguous fp32 [B, ...], nrm [B]"""
    _chk(x, f32, "x")
    _chk(g, f32, "g", x.shape)
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"dps_update: expected a non-empty [B, ...] tensor, got {tuple(x.shape)}")
    B = x.shape[0]
    _chk(nrm, f32, "nrm", (B,))
    for t, nme in ((g, "g"), (nrm, "nrm")):
        if t.device != x.device:
            raise ValueError(f"{nme}: expected a tensor on {x.device}, got {t.device}")
    scale = float(scale)
    if not (math.isfinite(scale) and scale >= 0.0):
        raise ValueError(f"dps_update: scale must be finite and >= 0, got {scale}")
    out = torch.empty_like(x)
    _lib.call("edm_dps_update", _p(x), _p(g), _p(nrm), scale, _p(out), B, x.numel() // B, _p(health(x.device)), _stream())
    return out


# ------------------------------------------------------------------ the input gradient of the denoiser (csrc/conv_in_dgrad.hip)
CONV_IN_DGRAD_MAX_CIMG = 8


def conv_in_dgrad_pack_cols(cimg: int) -> int:
    """columns of conv_in_dgrad's weight pack for `cimg` image channels (a host query, not a launch)"""
    return int(_lib.lib().edm_conv_in_dgrad_pack_cols(int(cimg)))


def conv_in_dgrad(gy, wpack, gD, sigma, sigma_data):
    """gx (fp32 NCHW [B, Cimg, H, W]) = c_in * dgrad3x3(gy; w^) [+ c_skip * gD]: the gradient of the denoiser's INPUT image from
    gy (bf16 NHWC [B, H, W, C0]: d loss / d conv_in's output; a 2-byte aligned view is accepted) and, optionally, the
    cotangent gD of D (fp32 NCHW like gx; the noisy * c_skip term of networks.py:602-603).  wpack: fp32 [C0, NT] from
    Conv2d.in_dgrad_pack(Cimg); Cimg = gD's channel count, else NT // 9.  fp32 accumulation, order-fixed, independent of B."""
    if not isinstance(gy, torch.Tensor) or not gy.is_cuda or gy.dtype != bf16 or gy.dim() != 4 or not gy.is_contiguous():
        raise ValueError("conv_in_dgrad: gy must be a contiguous bf16 (B, H, W, C0) GPU tensor")
    B, H, W, C0 = gy.shape
    _chk(wpack, f32, "wpack")
    if wpack.dim() != 2 or wpack.shape[0] != C0:
        raise ValueError(f"conv_in_dgrad: wpack must be (C0 = {C0}, NT), got {tuple(wpack.shape)}")
    NT = wpack.shape[1]
    if gD is not None:
        _chk(gD, f32, "gD")
        if gD.dim() != 4 or (gD.shape[0], gD.shape[2], gD.shape[3]) != (B, H, W):
            raise ValueError(f"conv_in_dgrad: gD {tuple(gD.shape)} does not match gy {tuple(gy.shape)}")
        cimg = gD.shape[1]
    else:
        cimg = NT // 9
    if not 1 <= cimg <= CONV_IN_DGRAD_MAX_CIMG or conv_in_dgrad_pack_cols(cimg) != NT:
        raise ValueError(f"conv_in_dgrad: {cimg} image channels do not match a pack of {NT} columns")
    if B < 1 or H < 1 or W < 1 or C0 < 1 or B > 65535:
        raise ValueError(f"conv_in_dgrad: bad shape {tuple(gy.shape)}")
    ss = _sigma_arg(sigma, B)
    for t, nme in ((wpack, "wpack"), (gD, "gD"), (sigma, "sigma")):
        if t is not None and t.device != gy.device:
            raise ValueError(f"{nme}: expected a tensor on {gy.device}, got {t.device}")
    gx = torch.empty(B, cimg, H, W, device=gy.device, dtype=f32)
    with _prof("conv_in_dgrad", 2.0 * B * H * W * C0 * 9 * cimg, 2.0 * gy.numel() + 4.0 * gx.numel() * (2 if gD is not None else 1)):
        _lib.call("edm_conv_in_dgrad", _p(gy), _p(wpack), _p(gD), _p(sigma), ss, float(sigma_data), _p(gx), B, cimg, H, W, C0,
                  _stream())
    return gx


# ------------------------------------------------------------------ likelihood and noise-level evaluation (csrc/sample_eval.hip)
NLL_MAX_PROBES = 32             # a probe is one bit of a Philox word
NLL_MAX_STEPS = 1 << 16         # step < 2**16 keeps the probe tags apart from the churn's and the blend's
NLL_MAX_CHUNKS = 64             # EDM_NLL_MAX_CHUNKS: per-sample partial sums of the order-fixed reduction


def _nll_batch(t, name, B, K, sample_shape, device):
    """an evaluation batch: contiguous fp32 [(1 + 2K) B, ...] on `device`"""
    _chk(t, f32, name, ((1 + 2 * K) * B,) + tuple(sample_shape))
    if t.device != device:
        raise ValueError(f"{name}: expected a tensor on {device}, got {t.device}")


def _nll_args(rec, x, step, K, **pos):
    _churn_rec(rec, x)
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= NLL_MAX_PROBES:
        raise ValueError(f"num_probes must be an integer in [1, {NLL_MAX_PROBES}], got {K!r}")
    if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < NLL_MAX_STEPS:
        raise ValueError(f"step must be an integer in [0, {NLL_MAX_STEPS}), got {step!r}")
    for name, v in pos.items():
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"{name} must be finite and > 0, got {v}")


def _nll_acc(L, B, device):
    _chk(L, torch.float64, "L", (B,))
    if L.device != device:
        raise ValueError(f"L: expected a tensor on {device}, got {L.device}")
    if B > 65535:
        raise ValueError(f"the likelihood kernels take at most 65535 samples per call, got {B}")
    return torch.empty(B * NLL_MAX_CHUNKS, dtype=torch.float64, device=device)


def nll_probe(x, h, rec, step, ev=0, num_probes=1):
    """The evaluation batch of the likelihood estimator: E = [x, x + h eps_0, x - h eps_0, x + h eps_1, ...] stacked along
    the batch, [(1 + 2K) B, ...] for K = num_probes Rademacher probes eps_p = +-1 drawn in the kernel (one bit of a Philox
    word each, under a tag of their own).  x: contiguous fp32 [B, ...]; h > 0; rec: the device record of ops.churn_record;
    step < 2**16 and ev in {0, 1} (the Euler evaluation of the step / its correction) select the stream.  The probes of
    sample b depend only on (seed, solve index, step, ev, probe, b, element)."""
    _chk(x, f32, "x")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"x: expected a non-empty [B, ...] tensor, got {tuple(x.shape)}")
    h = float(h)
    _nll_args(rec, x, step, num_probes, h=h)
    if ev not in (0, 1):
        raise ValueError(f"nll_probe: ev must be 0 or 1, got {ev!r}")
    B = x.shape[0]
    if B > 65535:
        raise ValueError(f"the likelihood kernels take at most 65535 samples per call, got {B}")
    E = torch.empty(((1 + 2 * num_probes) * B,) + tuple(x.shape[1:]), dtype=f32, device=x.device)
    _lib.call("edm_nll_probe", _p(x), h, _p(rec), step, int(ev), num_probes, B, x.numel() // B, _p(E),
              _p(health(x.device)), _stream())
    return E


def heun_euler_div(E, D, t0, t1, h0, h1, rec, step, L, num_probes=1):
    """heun_euler on the first B rows of the evaluation batch E and the network's output D on it, plus the divergence
    term: returns (dx [B, ...], E1) with E1 the evaluation batch of x1 (half-width h1, the probes of the step's
    correction), and adds (t1 - t0) / 2 * (CHW - q_b) / t0 to L (fp64 [B], in place), where
    q_b = mean_p sum_j eps_pj (D+_bj - D-_bj) / (2 h0) with the probes E was written with (ops.nll_probe(.., step, 0) or
    the previous heun_correct_div).  dx and E1[:B] equal ops.heun_euler(E[:B], D[:B], t0, t1) bit for bit."""
    _chk(E, f32, "E")
    K = num_probes
    t0, t1, h0, h1 = float(t0), float(t1), float(h0), float(h1)
    _nll_args(rec, E, step, K, t0=t0, h0=h0, h1=h1)
    if not math.isfinite(t1):
        raise ValueError(f"heun_euler_div: t1 must be finite, got {t1}")
    if E.dim() < 2 or E.numel() == 0 or E.shape[0] % (1 + 2 * K):
        raise ValueError(f"E: expected a non-empty [(1 + 2 * {K}) B, ...] tensor, got {tuple(E.shape)}")
    B = E.shape[0] // (1 + 2 * K)
    _nll_batch(D, "D", B, K, E.shape[1:], E.device)
    part = _nll_acc(L, B, E.device)
    dx = torch.empty((B,) + tuple(E.shape[1:]), dtype=f32, device=E.device)
    E1 = torch.empty_like(E)
    _lib.call("edm_heun_euler_div", _p(E), _p(D), t0, t1, h0, h1, _p(rec), step, K, B, E.numel() // E.shape[0], _p(dx),
              _p(E1), _p(part), _p(L), _p(health(E.device)), _stream())
    return dx, E1


def heun_correct_div(E, dx, E1, D1, t0, t1, h1, rec, step, L, num_probes=1, h_next=None):
    """heun_correct on the first B rows of (E, dx, E1) and the network's output D1 on E1, plus the divergence term: adds
    (t1 - t0) / 2 * (CHW - q_b) / t1 to L with q_b from D1 under the probes heun_euler_div wrote E1 with (half-width h1).
    With h_next it returns the evaluation batch of the new state for the next step's Euler evaluation (the probes of
    (step - 1, 0), half-width h_next; step >= 1); without, the new state alone, [B, ...].  Its first B rows equal
    ops.heun_correct(E[:B], dx, E1[:B], D1[:B], t0, t1) bit for bit."""
    _chk(E, f32, "E")
    K = num_probes
    t0, t1, h1 = float(t0), float(t1), float(h1)
    pos = dict(t1=t1, h1=h1)
    if h_next is not None:
        pos["h_next"] = h_next = float(h_next)
    _nll_args(rec, E, step, K, **pos)
    if not math.isfinite(t0):
        raise ValueError(f"heun_correct_div: t0 must be finite, got {t0}")
    if h_next is not None and step < 1:
        raise ValueError("heun_correct_div: h_next (probes for the next step) needs step >= 1")
    if E.dim() < 2 or E.numel() == 0 or E.shape[0] % (1 + 2 * K):
        raise ValueError(f"E: expected a non-empty [(1 + 2 * {K}) B, ...] tensor, got {tuple(E.shape)}")
    B = E.shape[0] // (1 + 2 * K)
    _nll_batch(E1, "E1", B, K, E.shape[1:], E.device)
    _nll_batch(D1, "D1", B, K, E.shape[1:], E.device)
    _chk(dx, f32, "dx", (B,) + tuple(E.shape[1:]))
    if dx.device != E.device:
        raise ValueError(f"dx: expected a tensor on {E.device}, got {dx.device}")
    part = _nll_acc(L, B, E.device)
    out = torch.empty_like(E) if h_next is not None else torch.empty_like(dx)
    _lib.call("edm_heun_correct_div", _p(E), _p(dx), _p(E1), _p(D1), t0, t1, h1, 1.0 if h_next is None else h_next,
              _p(rec), step, K, int(h_next is not None), B, E.numel() // E.shape[0], _p(out), _p(part), _p(L),
              _p(health(E.device)), _stream())
    return out


def nll_prior(x, t, L):
    """L_b += log N(x_b; 0, t^2 I) in nats, summed in fp64 in a fixed order.  x: contiguous fp32 [B, ...]; L: fp64 [B]."""
    _chk(x, f32, "x")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"x: expected a non-empty [B, ...] tensor, got {tuple(x.shape)}")
    t = float(t)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"nll_prior: t must be finite and > 0, got {t}")
    B = x.shape[0]
    part = _nll_acc(L, B, x.device)
    _lib.call("edm_nll_prior", _p(x), t, B, x.numel() // B, _p(part), _p(L), _p(health(x.device)), _stream())
    return L


EVAL_MAX_LEVELS = 65535         # a level is the low half of the Philox tag 0x45560000 ^ level


def _chk_eval(t, dtype, name, shape=None, device=None):
    """_chk for the loss-by-noise-level ops: every bad operand is a ValueError"""
    try:
        _chk(t, dtype, name, shape)
    except (TypeError, RuntimeError) as e:
        raise ValueError(str(e)) from None
    if device is not None and t.device != device:
        raise ValueError(f"{name}: expected a tensor on {device}, got {t.device}")


def _eval_diffuse_args(clean, ids, level, sigmas, rec, check_levels):
    """the operand checks eval_diffuse and eval_diffuse_classes share -> (pairs, levels)"""
    _chk_eval(clean, f32, "clean")
    if clean.dim() < 2 or clean.numel() == 0:
        raise ValueError(f"clean: expected a non-empty [B, ...] tensor, got {tuple(clean.shape)}")
    B = clean.shape[0]
    _chk_eval(ids, torch.uint32, "ids", (B,), clean.device)
    _chk_eval(level, torch.int32, "level", (B,), clean.device)
    _chk_eval(sigmas, f32, "sigmas", None, clean.device)
    if sigmas.dim() != 1 or not 1 <= sigmas.numel() <= EVAL_MAX_LEVELS:
        raise ValueError(f"sigmas: expected 1 to {EVAL_MAX_LEVELS} levels in a 1-d tensor, got {tuple(sigmas.shape)}")
    try:
        _churn_rec(rec, clean)
    except (TypeError, RuntimeError) as e:
        raise ValueError(str(e)) from None
    L = sigmas.numel()
    if check_levels:
        lo, hi = (int(v) for v in torch.aminmax(level))
        if lo < 0 or hi >= L:
            raise ValueError(f"level: values must be in [0, {L}), got [{lo}, {hi}]")
    return B, L


def eval_diffuse(clean, ids, level, sigmas, rec, check_levels=True):
    """noisy_b = clean_b + sigmas[level[b]] * n with n ~ N(0, 1) drawn in the kernel for the IMAGE ids[b]: the noise depends
    only on (seed, draw, ids[b], level[b], element), not on the batch or the row.  clean: contiguous fp32 [B, ...]; ids:
    uint32 [B]; level: int32 [B] with values in [0, L); sigmas: fp32 [L], L <= 65535; rec: ops.churn_record(seed, draw).
    Returns (noisy, sigma [B] fp32).  The level range is checked on the host before the launch (one device read);
    check_levels=False is for a caller that built `level` itself from values it has already checked."""
    B, L = _eval_diffuse_args(clean, ids, level, sigmas, rec, check_levels)
    noisy = torch.empty_like(clean)
    sigma = torch.empty(B, dtype=f32, device=clean.device)
    _lib.call("edm_eval_diffuse", _p(clean), _p(ids), _p(level), _p(sigmas), L, _p(rec), B, clean.numel() // B,
              _p(noisy), _p(sigma), _p(health(clean.device)), _stream())
    return noisy, sigma


def eval_sqerr(D, clean, out=None):
    """se[b] = sum_j ((double)D_bj - (double)clean_bj)^2 in fp64, summed in an order that depends on the sample size
    alone: the bits of se[b] do not depend on the batch.  D, clean: contiguous fp32 [B, ...], B <= 65535; out: a
    contiguous fp64 [B] tensor (a slice of a result matrix) that is written, or None to allocate."""
    _chk_eval(clean, f32, "clean")
    if clean.dim() < 2 or clean.numel() == 0:
        raise ValueError(f"clean: expected a non-empty [B, ...] tensor, got {tuple(clean.shape)}")
    _chk_eval(D, f32, "D", clean.shape, clean.device)
    B = clean.shape[0]
    if B > 65535:
        raise ValueError(f"eval_sqerr takes at most 65535 samples per call, got {B}")
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=clean.device)
    else:
        _chk_eval(out, torch.float64, "out", (B,), clean.device)
    part = torch.empty(B * NLL_MAX_CHUNKS, dtype=torch.float64, device=clean.device)
    _lib.call("edm_eval_sqerr", _p(D), _p(clean), B, clean.numel() // B, _p(part), _p(out), _p(health(clean.device)),
              _stream())
    return out


def _chk_classes(num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
        raise ValueError(f"num_classes must be an integer >= 1, got {num_classes!r}")
    return num_classes


def eval_diffuse_classes(clean, ids, level, sigmas, rec, num_classes, check_levels=True):
    """eval_diffuse for the class sweep: the noise of pair p is drawn once and stored to the C = num_classes rows
    p * C + c of the result, so every class of an (image, level, draw) meets the same noise and no replicated `clean`
    exists in memory.  clean: contiguous fp32 [P, ...]; ids, level: [P] as eval_diffuse.  Returns (noisy [P * C, ...],
    sigma [P * C]); row p * C + c holds the bits eval_diffuse gives for pair p."""
    C = _chk_classes(num_classes)
    P, L = _eval_diffuse_args(clean, ids, level, sigmas, rec, check_levels)
    if P * C >= 1 << 31:
        raise ValueError(f"eval_diffuse_classes: P * num_classes must be below 2**31, got {P} * {C}")
    noisy = torch.empty((P * C,) + tuple(clean.shape[1:]), dtype=f32, device=clean.device)
    sigma = torch.empty(P * C, dtype=f32, device=clean.device)
    _lib.call("edm_eval_diffuse_classes", _p(clean), _p(ids), _p(level), _p(sigmas), L, _p(rec), P, C,
              clean.numel() // P, _p(noisy), _p(sigma), _p(health(clean.device)), _stream())
    return noisy, sigma


def eval_sqerr_classes(D, clean, num_classes, out=None):
    """eval_sqerr for the class sweep: se[p * C + c] = sum_j ((double)D[p * C + c]_j - (double)clean[p]_j)^2 with the bits
    eval_sqerr gives for that row against clean[p]; `clean` [P, ...] is read in place, never replicated.  D: contiguous
    fp32 [P * C, ...], P * C <= 65535; out: a contiguous fp64 [P * C] tensor that is written, or None to allocate."""
    _chk_eval(clean, f32, "clean")
    if clean.dim() < 2 or clean.numel() == 0:
        raise ValueError(f"clean: expected a non-empty [P, ...] tensor, got {tuple(clean.shape)}")
    C = _chk_classes(num_classes)
    P = clean.shape[0]
    rows = P * C
    if rows > 65535:
        raise ValueError(f"eval_sqerr_classes takes at most 65535 rows per call, got {P} * {C}")
    _chk_eval(D, f32, "D", (rows,) + tuple(clean.shape[1:]), clean.device)
    if out is None:
        out = torch.empty(rows, dtype=torch.float64, device=clean.device)
    else:
        _chk_eval(out, torch.float64, "out", (rows,), clean.device)
    part = torch.empty(rows * NLL_MAX_CHUNKS, dtype=torch.float64, device=clean.device)
    _lib.call("edm_eval_sqerr_classes", _p(D), _p(clean), P, C, clean.numel() // P, _p(part), _p(out),
              _p(health(clean.device)), _stream())
    return out


# ------------------------------------------------------------------ adaptive ODE solver (csrc/adaptive.hip)
ADAPT_ROWS = 8                  # EDM_ADAPT_ROWS: 32-bit words of per-sample state of the adaptive solver
ADAPT_ACTIVE, ADAPT_DONE, ADAPT_FAILED = 0, 1, 2


class AdaptRows(types.SimpleNamespace):
    """the rows of an adaptive solver's device state as [B] views that share its memory: t, t1, h, err (fp32), status,
    accepted, rejected, after_reject (int32 holding the uint32 bits)"""


def adapt_rows(state) -> AdaptRows:
    _adapt_state(state, 0, None)
    f = state.view(f32)
    return AdaptRows(t=f[0], t1=f[1], h=f[2], err=f[3], status=state[4], accepted=state[5], rejected=state[6],
                     after_reject=state[7])


def _adapt_state(state, B, device):
    _chk_eval(state, torch.int32, "state", None, device)
    if state.dim() != 2 or state.shape[0] != ADAPT_ROWS or state.shape[1] < 1 or (B and state.shape[1] != B):
        raise ValueError(f"state: expected an int32 [{ADAPT_ROWS}, {B or 'B'}] tensor (ops.adapt_begin), got "
                         f"{tuple(state.shape)}")


def _adapt_batch(x, name="x"):
    _chk_eval(x, f32, name)
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty [B, ...] tensor, got {tuple(x.shape)}")
    return x.shape[0], x.numel() // x.shape[0]


def _adapt_times(t, t1, B, device):
    for v, name in ((t, "t"), (t1, "t1")):
        _chk_eval(v, f32, name, (B,), device)


def adapt_begin(B, t_start, t_end, h0, device):
    """The device state of an adaptive solve of B samples from t_start to t_end (both > 0) with the first proposal h0
    (signed, pointing at t_end): an int32 [ADAPT_ROWS, B] tensor (ops.adapt_rows names its rows)."""
    if isinstance(B, bool) or not isinstance(B, int) or B < 1:
        raise ValueError(f"adapt_begin: B must be a positive integer, got {B!r}")
    t_start, t_end, h0 = float(t_start), float(t_end), float(h0)
    if not (all(math.isfinite(v) for v in (t_start, t_end, h0)) and t_start > 0 and t_end > 0 and t_start != t_end):
        raise ValueError(f"adapt_begin: t_start and t_end must be finite, > 0 and different, got {t_start}, {t_end}")
    if h0 == 0.0 or (h0 > 0) != (t_end > t_start):
        raise ValueError(f"adapt_begin: h0 must be non-zero and point from t_start to t_end, got {h0}")
    state = torch.empty((ADAPT_ROWS, B), dtype=torch.int32, device=device)
    _adapt_state(state, B, None)            # (a host tensor ends here: there is no CPU path)
    _lib.call("edm_adapt_begin", t_start, t_end, h0, B, _p(state), _stream())
    return state


def adapt_euler(x, D, t, t1):
    """heun_euler with the times of sample b read from t[b], t1[b] (fp32 [B] on the device): (dx, x1).  A sample with
    t1[b] == t[b] gets x1 = x and dx = 0 whatever D holds."""
    B, CHW = _adapt_batch(x)
    _chk_eval(D, f32, "D", x.shape, x.device)
    _adapt_times(t, t1, B, x.device)
    dx, x1 = torch.empty_like(x), torch.empty_like(x)
    _lib.call("edm_adapt_euler", _p(x), _p(D), _p(t), _p(t1), B, CHW, _p(dx), _p(x1), _p(health(x.device)), _stream())
    return dx, x1


def adapt_correct(x, dx, x1, D1, t, t1, atol, rtol, part=None):
    """heun_correct with per-sample times, and the error partials of the step: returns (y, part) with part an fp64
    [B, NLL_MAX_CHUNKS] workspace whose row b holds, in its first chunks, the order-fixed partial sums of
    ((y - x1) / (atol + rtol max(|x|, |y|)))^2 over sample b (adapt_control adds them up)."""
    B, CHW = _adapt_batch(x)
    if B > 65535:
        raise ValueError(f"adapt_correct takes at most 65535 samples per call, got {B}")
    for v, name in ((dx, "dx"), (x1, "x1"), (D1, "D1")):
        _chk_eval(v, f32, name, x.shape, x.device)
    _adapt_times(t, t1, B, x.device)
    atol, rtol = float(atol), float(rtol)
    if not (math.isfinite(atol) and math.isfinite(rtol) and atol >= 0 and rtol >= 0 and atol + rtol > 0):
        raise ValueError(f"adapt_correct: atol and rtol must be finite, >= 0 and not both 0, got {atol}, {rtol}")
    if part is None:
        part = torch.empty((B, NLL_MAX_CHUNKS), dtype=torch.float64, device=x.device)
    else:
        _chk_eval(part, torch.float64, "part", (B, NLL_MAX_CHUNKS), x.device)
    y = torch.empty_like(x)
    _lib.call("edm_adapt_correct", _p(x), _p(dx), _p(x1), _p(D1), _p(t), _p(t1), B, CHW, atol, rtol, _p(y), _p(part),
              _p(health(x.device)), _stream())
    return y, part


def adapt_chunks(CHW: int) -> int:
    """how many entries of a row of `part` a sample of CHW elements fills (a function of CHW alone): the rule the kernels
    index with, asked of the library (edm_sample_chunks; host logic, no launch)"""
    return int(_lib.call("edm_sample_chunks", int(CHW)))


def adapt_control(part, CHW, state, t_end, active, *, safety=0.9, fac_min=0.2, fac_max=5.0, h_floor=1e-6, accept=None):
    """The step controller, one thread per sample in fp64: E from `part`, accept iff E <= 1, the next h, t and t1 written
    to `state`, counters updated (see include/tinyedm_hip.h).  Returns the accept flags, uint8 [B]; adds the number of
    samples still active to `active`, a one-element int32 tensor on the device."""
    _adapt_state(state, 0, None)
    B = state.shape[1]
    _chk_eval(part, torch.float64, "part", (B, NLL_MAX_CHUNKS), state.device)
    _chk_eval(active, torch.int32, "active", None, state.device)
    if active.numel() != 1:
        raise ValueError(f"active: expected a one-element int32 tensor, got {tuple(active.shape)}")
    if isinstance(CHW, bool) or not isinstance(CHW, int) or CHW < 1:
        raise ValueError(f"adapt_control: CHW must be a positive integer, got {CHW!r}")
    t_end, safety, fac_min, fac_max, h_floor = (float(v) for v in (t_end, safety, fac_min, fac_max, h_floor))
    check_controller(safety, fac_min, fac_max, h_floor)
    if not (math.isfinite(t_end) and t_end > 0):
        raise ValueError(f"adapt_control: t_end must be finite and > 0, got {t_end}")
    if accept is None:
        accept = torch.empty(B, dtype=torch.uint8, device=state.device)
    else:
        _chk_eval(accept, torch.uint8, "accept", (B,), state.device)
    _lib.call("edm_adapt_control", _p(part), B, CHW, t_end, safety, fac_min, fac_max, h_floor, _p(state), _p(accept),
              _p(active), _p(health(state.device)), _stream())
    return accept


def check_controller(safety, fac_min, fac_max, h_floor=0.0) -> None:
    """the controller constants of the adaptive solver, on the host"""
    vals = (safety, fac_min, fac_max, h_floor)
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) for v in vals):
        raise ValueError(f"adaptive controller: safety, fac_min, fac_max and h_floor must be finite numbers, got {vals}")
    if not (0 < safety <= 1 and 0 < fac_min < 1 <= fac_max and 0 <= h_floor < 1):
        raise ValueError(f"adaptive controller: needs 0 < safety <= 1, 0 < fac_min < 1 <= fac_max and 0 <= h_floor < 1, "
                         f"got safety={safety}, fac_min={fac_min}, fac_max={fac_max}, h_floor={h_floor}")


def adapt_commit(x, y, accept):
    """x <- accept[b] ? y : x in place; a sample that was not accepted is not written.  Returns x."""
    B, CHW = _adapt_batch(x)
    _chk_eval(y, f32, "y", x.shape, x.device)
    _chk_eval(accept, torch.uint8, "accept", (B,), x.device)
    if x.data_ptr() == y.data_ptr():
        raise ValueError("adapt_commit: y must not alias x")
    _lib.call("edm_adapt_commit", _p(x), _p(y), _p(accept), B, CHW, _stream())
    return x


# ------------------------------------------------------------------ parallel-in-time sampling (csrc/picard.hip)
PICARD_ROWS = 3                 # EDM_PICARD_ROWS: 32-bit words of per-sample state of the parallel solver
PICARD_MAX_WINDOW = 64          # EDM_PICARD_MAX_WINDOW
PICARD_ACTIVE, PICARD_DONE = 0, 1


class PicardRows(types.SimpleNamespace):
    """the rows of a parallel solver's device state as [B] int32 views that share its memory: start (the table index of
    window position 0), status, iterations"""


def picard_rows(state) -> PicardRows:
    _picard_state(state, 0, None)
    return PicardRows(start=state[0], status=state[1], iterations=state[2])


def _picard_state(state, B, device):
    _chk_eval(state, torch.int32, "state", None, device)
    if state.dim() != 2 or state.shape[0] != PICARD_ROWS or state.shape[1] < 1 or (B and state.shape[1] != B):
        raise ValueError(f"state: expected an int32 [{PICARD_ROWS}, {B or 'B'}] tensor (ops.picard_begin), got "
                         f"{tuple(state.shape)}")


def _picard_dims(who, N, P):
    if isinstance(N, bool) or not isinstance(N, int) or N < 2:
        raise ValueError(f"{who}: N (the table's steps) must be an integer >= 2, got {N!r}")
    if isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= PICARD_MAX_WINDOW:
        raise ValueError(f"{who}: the window must be an integer in 1 .. {PICARD_MAX_WINDOW}, got {P!r}")


def _picard_window(X, name="X"):
    """(P, B, CHW) of a window buffer [P + 1, B, ...]"""
    _chk_eval(X, f32, name)
    if X.dim() < 3 or X.shape[0] < 2 or X.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty [P + 1, B, ...] window buffer, got {tuple(X.shape)}")
    P, B = X.shape[0] - 1, X.shape[1]
    if B > 65535:
        raise ValueError(f"{name}: at most 65535 samples per call, got {B}")
    return P, B, X.numel() // (X.shape[0] * B)


def _picard_rows_of(v, name, P, B, CHW, device):
    """a [P][B][CHW] operand, in whatever shape (the [P * B, C, H, W] of a network batch, for one)"""
    _chk_eval(v, f32, name, None, device)
    if v.numel() != P * B * CHW:
        raise ValueError(f"{name}: expected {P} x {B} rows of {CHW} elements, got {tuple(v.shape)}")


def picard_chunks(CHW: int) -> int:
    """how many partials per window position a sample of CHW elements fills (a function of CHW alone; = adapt_chunks)"""
    return adapt_chunks(CHW)


def picard_tol(atol, rtol, device, out=None):
    """{atol, rtol} as the fp64 [2] device tensor picard_scan reads (a captured iteration re-reads it at every replay)"""
    for name, v in (("atol", atol), ("rtol", rtol)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"picard: {name} must be a finite number >= 0, got {v!r}")
    host = torch.tensor([float(atol), float(rtol)], dtype=torch.float64)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=device)
    _chk_eval(out, torch.float64, "tol", (2,), None)
    out.copy_(host)
    return out


def picard_begin(x0, t_table, N, P, *, X=None, T=None, state=None):
    """The empty window at the head of the table: (X, T, state) with X[j] = t_j x0 for j = 0 .. min(P, N - 1) (one
    rounding: X[0] is the table solver's first state bit for bit, the rest is the first guess x_j = X[0] t_j / t_0), copies
    of X[0] past the table's end, T[j][b] = t[min(j, N - 1)] and every sample active at start 0.  x0: fp32 [B, ...] unit
    noise; t_table: the fp32 sigma table on the device, at least N entries."""
    _picard_dims("picard_begin", N, P)
    B, CHW = _adapt_batch(x0, "x0")
    if B > 65535:
        raise ValueError(f"picard_begin: at most 65535 samples per call, got {B}")
    _chk_eval(t_table, f32, "t_table", None, x0.device)
    if t_table.dim() != 1 or t_table.numel() < N:
        raise ValueError(f"t_table: expected a 1-d table of at least {N} entries, got {tuple(t_table.shape)}")
    shape = (P + 1, *x0.shape)
    if X is None:
        X = torch.empty(shape, dtype=f32, device=x0.device)
    else:
        _chk_eval(X, f32, "X", shape, x0.device)
    if T is None:
        T = torch.empty((P + 1, B), dtype=f32, device=x0.device)
    else:
        _chk_eval(T, f32, "T", (P + 1, B), x0.device)
    if state is None:
        state = torch.empty((PICARD_ROWS, B), dtype=torch.int32, device=x0.device)
    _picard_state(state, B, x0.device)
    _lib.call("edm_picard_slide", _p(x0), None, None, _p(state), _p(t_table), 1, B, N, P, CHW, _p(X), _p(T), _stream())
    return X, T, state


def picard_scan(X, dx, X1, D1, T, state, atol=None, rtol=None, *, N, tol=None, Xnew=None, part=None):
    """The prefix sum of one Picard iteration: (Xnew, part).  Xnew[0] = X[0], Xnew[j + 1] = fma(t1 - t0, slope_j, Xnew[j])
    over the live positions with slope_j = 0.5 dx_j + 0.5 (X1_j - D1_j) / t1 from the old iterate (D1 None: slope_j = dx_j,
    the Euler iteration), inactive positions copy the last live one.  part: fp64 [B, P, picard_chunks(CHW)], the
    order-fixed partial sums of ((new - old) / (atol + rtol max(|old|, |new|)))^2 per position (picard_control adds them
    up).  The tolerances are read from `tol` (ops.picard_tol) when given, else from atol and rtol."""
    P, B, CHW = _picard_window(X)
    _picard_dims("picard_scan", N, P)
    _picard_rows_of(dx, "dx", P, B, CHW, X.device)
    if D1 is not None:
        _picard_rows_of(X1, "X1", P, B, CHW, X.device)
        _picard_rows_of(D1, "D1", P, B, CHW, X.device)
    _chk_eval(T, f32, "T", (P + 1, B), X.device)
    _picard_state(state, B, X.device)
    if tol is None:
        tol = picard_tol(atol, rtol, X.device)
    else:
        _chk_eval(tol, torch.float64, "tol", (2,), X.device)
    if Xnew is None:
        Xnew = torch.empty_like(X)
    else:
        _chk_eval(Xnew, f32, "Xnew", X.shape, X.device)
        if Xnew.data_ptr() == X.data_ptr():
            raise ValueError("picard_scan: Xnew must not alias X")
    pshape = (B, P, picard_chunks(CHW))
    if part is None:
        part = torch.empty(pshape, dtype=torch.float64, device=X.device)
    else:
        _chk_eval(part, torch.float64, "part", pshape, X.device)
    _lib.call("edm_picard_scan", _p(X), _p(dx), _p(X1 if D1 is not None else None), _p(D1), _p(T), _p(state), _p(tol), B, N,
              P, CHW, _p(Xnew), _p(part), _p(health(X.device)), _stream())
    return Xnew, part


def picard_control(part, CHW, state, N, P, active, *, stride=None, err=None):
    """The window controller, one thread per sample in fp64: E_j of the live positions from `part`, the stride
    min(leading converged + 1, live), the state advanced (see include/tinyedm_hip.h).  Returns the strides, int32 [B] (0
    for a sample that was not active); adds the number of samples still active to `active`, a one-element int32 device
    tensor.  err: optional fp64 [B, P] that receives E of the live positions."""
    _picard_state(state, 0, None)
    B = state.shape[1]
    _picard_dims("picard_control", N, P)
    if isinstance(CHW, bool) or not isinstance(CHW, int) or CHW < 1:
        raise ValueError(f"picard_control: CHW must be a positive integer, got {CHW!r}")
    _chk_eval(part, torch.float64, "part", (B, P, picard_chunks(CHW)), state.device)
    _chk_eval(active, torch.int32, "active", None, state.device)
    if active.numel() != 1:
        raise ValueError(f"active: expected a one-element int32 tensor, got {tuple(active.shape)}")
    if stride is None:
        stride = torch.empty(B, dtype=torch.int32, device=state.device)
    else:
        _chk_eval(stride, torch.int32, "stride", (B,), state.device)
    if err is not None:
        _chk_eval(err, torch.float64, "err", (B, P), state.device)
    _lib.call("edm_picard_control", _p(part), B, CHW, N, P, _p(state), _p(stride), _p(err), _p(active), _stream())
    return stride


def picard_slide(Xnew, D, stride, state, t_table, *, N, X=None, T=None):
    """Slide every sample's window by its stride: (X, T), X another buffer than Xnew.  X[j] = Xnew[j + stride] while that
    is a computed position; a position entering the window at table index i <= N - 1 is extrapolated along the ODE's
    solution for a frozen denoised image, fma(Xnew[L] - Dh, t_i / t_{s + L}, Dh) with Dh = D[L - 1]; indices past N - 1 copy
    Xnew[L].  T is rewritten from the state, which picard_control has advanced already."""
    P, B, CHW = _picard_window(Xnew, "Xnew")
    _picard_dims("picard_slide", N, P)
    _picard_rows_of(D, "D", P, B, CHW, Xnew.device)
    _chk_eval(stride, torch.int32, "stride", (B,), Xnew.device)
    _picard_state(state, B, Xnew.device)
    _chk_eval(t_table, f32, "t_table", None, Xnew.device)
    if t_table.dim() != 1 or t_table.numel() < N:
        raise ValueError(f"t_table: expected a 1-d table of at least {N} entries, got {tuple(t_table.shape)}")
    if X is None:
        X = torch.empty_like(Xnew)
    else:
        _chk_eval(X, f32, "X", Xnew.shape, Xnew.device)
        if X.data_ptr() == Xnew.data_ptr():
            raise ValueError("picard_slide: X must not alias Xnew (ping-pong, never in place)")
    if T is None:
        T = torch.empty((P + 1, B), dtype=f32, device=Xnew.device)
    else:
        _chk_eval(T, f32, "T", (P + 1, B), Xnew.device)
    _lib.call("edm_picard_slide", _p(Xnew), _p(D), _p(stride), _p(state), _p(t_table), 0, B, N, P, CHW, _p(X), _p(T),
              _stream())
    return X, T


# ------------------------------------------------------------------ reference-precision evaluation (csrc/eval_f32.hip)
def _nhwc32(t, name):
    _chk(t, f32, name)
    if t.dim() != 4:
        raise ValueError(f"{name}: expected (B,H,W,C)")
    return t.shape


def f32_conv(x, w_hat, taps, residual=None, alpha=1.0, beta=0.0, lin=None, gain=None):
    """x (B,H,W,Cin) fp32 NHWC, w_hat (Cout, I*taps) fp32 (master OIHW order, I <= Cin) -> (B,H,W,Cout) fp32:
    alpha*conv + beta*residual, or with lin/gain the block's modulation epilogue mp_silu(alpha*conv*(lin*gain+1))."""
    B, H, W, Cin = _nhwc32(x, "x")
    _chk(w_hat, f32, "w_hat")
    if w_hat.dim() != 2 or w_hat.shape[1] % taps:
        raise ValueError(f"f32_conv: w_hat {tuple(w_hat.shape)} does not match taps={taps}")
    Cout, I = w_hat.shape[0], w_hat.shape[1] // taps
    if I > Cin:
        raise ValueError(f"f32_conv: weight has {I} input channels, x only {Cin}")
    if residual is not None:
        _chk(residual, f32, "residual", (B, H, W, Cout))
    ls = 0
    if lin is not None:
        ls = _lin_view(lin, B, Cout, "lin")
        _chk(gain, f32, "gain")
    y = torch.empty(B, H, W, Cout, device=x.device, dtype=f32)
    with _prof("f32_conv3x3" if taps == 9 else "f32_conv1x1", 2.0 * B * H * W * I * Cout * taps,
               4.0 * (B * H * W * (Cin + Cout * (2 if residual is not None else 1)) + w_hat.numel())):
        _lib.call("edm_f32_conv", _p(x), _p(w_hat), _p(y), _p(residual), float(alpha), float(beta), _p(lin), ls, _p(gain),
                  B, H, W, Cin, I, Cout, taps, _stream())
    return y


def f32_to_pairs(x):
    """(B,H,W,C) fp32 -> (B,H,W,2C) bf16 = [hi | lo], hi = bf16(x), lo = bf16(x - hi): the operand format of split_conv"""
    B, H, W, C = _nhwc32(x, "x")
    if C % 8:
        raise ValueError("f32_to_pairs: C % 8 required")
    p = torch.empty(B, H, W, 2 * C, device=x.device, dtype=bf16)
    _lib.call("edm_f32_to_pairs", _p(x), _p(p), B * H * W, C, _stream())
    return p


def split_pack(w_hat, taps, out=None):
    """w_hat (Cout, I*taps) fp32 -> (taps, Cout, 3*Ip) bf16 = [w_hi | w_lo | w_hi], Ip = I rounded up to 32.
    out: rewrite this buffer in place (the persistent pack of a weight-prep plan: a captured solve keeps its address)"""
    _chk(w_hat, f32, "w_hat")
    Cout, I = w_hat.shape[0], w_hat.shape[1] // taps
    Ip = (I + 31) // 32 * 32
    pk = torch.empty(taps, Cout, 3 * Ip, device=w_hat.device, dtype=bf16) if out is None else \
        _chk(out, bf16, "out", (taps, Cout, 3 * Ip))
    _lib.call("edm_split_pack", _p(w_hat), _p(pk), Cout, I, taps, Ip, _stream())
    return pk


def split_conv_fold_supported(xp_shape, Cout, C2):
    """split_conv(fold=) covers this 3x3 shape ((B, H, W, 2C) pairs -> Cout) with a C2-channel projection riding along"""
    B, H, W, C2x = xp_shape
    C = C2x // 2
    return bool(FOLD_PROJ and C % 64 == 0 and C2 % 32 == 0 and
                _lib.call("edm_conv3x3_fold_supported", B, H, W, 3 * C, Cout, 3 * C2))


def split_conv(xp, pack3, taps, residual=None, alpha=1.0, beta=0.0, lin=None, gain=None, pairs_out=False, also_pairs=False,
               dest=None, silu_pairs=False, fold=None):
    """fp32-accurate conv in three bf16 MFMA passes: xp (B,H,W,2C) bf16 pairs (f32_to_pairs), pack3 (taps,Cout,3C) bf16
    (split_pack) -> (B,H,W,Cout) fp32 = alpha*conv + beta*residual, or with lin/gain mp_silu(alpha*conv*(lin*gain+1));
    pairs_out=True: the result comes back as (B,H,W,2Cout) bf16 pairs instead (it only feeds another split_conv);
    also_pairs=True: (fp32 result, the same as pairs) from the one launch;
    silu_pairs=True: (fp32 result, mp_silu of it as pairs): what a decoder block without a skip reads (networks.py:313-316);
    dest=(cat, sil): (B,H,W,2 Ct) bf16 pairs buffers of the NEXT decoder block's concatenated operands, Ct > Cout: the result
    and mp_silu of it are written into their left column blocks (hi at columns [0, Cout), lo at [Ct, Ct + Cout)) and nothing
    else; returns cat (f32_skip_half fills the right blocks)."""
    B, H, W, C2 = _nhwc(xp, "xp")
    C = C2 // 2
    _chk(pack3, bf16, "pack3")
    if pack3.dim() != 3 or pack3.shape[0] != taps or pack3.shape[2] != 3 * C or C % 32:
        raise ValueError(f"split_conv: pack {tuple(pack3.shape)} does not match taps={taps}, C={C} (C % 32 required)")
    Cout = pack3.shape[1]
    if residual is not None:
        _chk(residual, f32, "residual", (B, H, W, Cout))
    ls = 0
    if lin is not None:
        ls = _lin_view(lin, B, Cout, "lin")
        _chk(gain, f32, "gain")
    if sum(map(bool, (pairs_out, also_pairs, dest is not None, silu_pairs))) > 1:
        raise ValueError("split_conv: pairs_out / also_pairs / silu_pairs / dest exclude one another")
    if fold is not None:
        # fold = (x2p, pack3_1x1): alpha * conv3x3(xp) + beta * conv1x1(x2p) in one launch (the decoder's skip projection,
        # edm_split_conv_fold); `beta` is the projection's coefficient, there is no residual
        x2p, pk1 = fold
        if residual is not None or lin is not None or taps != 9:
            raise ValueError("split_conv: fold excludes residual / modulation and needs taps == 9")
        B2, H2, W2, C22 = _nhwc(x2p, "fold[0]")
        C2 = C22 // 2
        _chk(pk1, bf16, "fold[1]", (1, Cout, 3 * C2))
        if (B2, H2, W2) != (B, H, W):
            raise ValueError("split_conv: fold operand shape mismatch")
        y = yp = ys = None
        ld = lo = 0
        ret = None
        if dest is not None:
            cat, sil = dest
            Ct = cat.shape[-1] // 2
            _chk(cat, bf16, "dest[0]", (B, H, W, 2 * Ct))
            if sil is not None:
                _chk(sil, bf16, "dest[1]", (B, H, W, 2 * Ct))
            if Ct <= Cout or Ct % 4:
                raise ValueError("split_conv: dest must be wider than the result")
            yp, ys, ld, lo, ret = cat, sil, 2 * Ct, Ct, cat
        elif pairs_out:
            ret = yp = torch.empty(B, H, W, 2 * Cout, device=xp.device, dtype=bf16)
        else:
            y = torch.empty(B, H, W, Cout, device=xp.device, dtype=f32)
            if also_pairs or silu_pairs:
                p2 = torch.empty(B, H, W, 2 * Cout, device=xp.device, dtype=bf16)
                yp, ys = (p2, None) if also_pairs else (None, p2)
                ret = (y, p2)
            else:
                ret = y
        with _prof("split_conv3x3_fold", 2.0 * B * H * W * Cout * (9 * C + C2), 4.0 * B * H * W * (C + C2 + Cout) + 2.0 * pack3.numel()):
            _lib.call("edm_split_conv_fold", _p(xp), _p(pack3), _p(x2p), _p(pk1), C2, _p(y), _p(yp), ld, lo, _p(ys), float(alpha),
                      float(beta), B, H, W, C, Cout, _stream())
        return ret
    nb = 4.0 * B * H * W * (C + Cout * (2 if residual is not None else 1)) + 2.0 * pack3.numel()
    pname = "split_conv3x3" if taps == 9 else "split_conv1x1"
    if dest is not None or also_pairs or silu_pairs:
        y = yp = ys = None
        ld = lo = 0
        if dest is not None:
            cat, sil = dest
            Ct = cat.shape[-1] // 2
            _chk(cat, bf16, "dest[0]", (B, H, W, 2 * Ct))
            if sil is not None:
                _chk(sil, bf16, "dest[1]", (B, H, W, 2 * Ct))
            if Ct <= Cout or Ct % 4:
                raise ValueError("split_conv: dest must be wider than the result")
            yp, ys, ld, lo = cat, sil, 2 * Ct, Ct
        else:
            y = torch.empty(B, H, W, Cout, device=xp.device, dtype=f32)
            p2 = torch.empty(B, H, W, 2 * Cout, device=xp.device, dtype=bf16)
            yp, ys = (p2, None) if also_pairs else (None, p2)
        with _prof(pname, 2.0 * B * H * W * C * Cout * taps, nb):
            _lib.call("edm_split_conv_o", _p(xp), _p(pack3), _p(y), _p(yp), ld, lo, _p(ys), _p(residual), float(alpha),
                      float(beta), _p(lin), ls, _p(gain), B, H, W, C, Cout, taps, _stream())
        return cat if dest is not None else (y, p2)
    y = None if pairs_out else torch.empty(B, H, W, Cout, device=xp.device, dtype=f32)
    yp = torch.empty(B, H, W, 2 * Cout, device=xp.device, dtype=bf16) if pairs_out else None
    with _prof(pname, 2.0 * B * H * W * C * Cout * taps, nb):
        _lib.call("edm_split_conv", _p(xp), _p(pack3), _p(y), _p(yp), _p(residual), float(alpha), float(beta), _p(lin), ls,
                  _p(gain), B, H, W, C, Cout, taps, _stream())
    return yp if pairs_out else y


def f32_skip_half(skip, gate, cat, sil=None):
    """cat[..., Ci:Ct] (hi) / [Ct+Ci:2Ct] (lo) = pairs of skip*gate, sil likewise of mp_silu(skip*gate): the skip half of the
    split evaluation's concatenated operands (the input half: split_conv(dest=))"""
    B, H, W, Cs = _nhwc32(skip, "skip")
    _chk(gate, f32, "gate", (B, Cs))
    Ct = cat.shape[-1] // 2
    _chk(cat, bf16, "cat", (B, H, W, 2 * Ct))
    if sil is not None:
        _chk(sil, bf16, "sil", (B, H, W, 2 * Ct))
    if Ct <= Cs:
        raise ValueError("f32_skip_half: cat must be wider than the skip")
    _lib.call("edm_f32_skip_half", _p(skip), _p(gate), _p(cat), _p(sil), B, H * W, Ct - Cs, Cs, _stream())


def f32_pool_pixelnorm_silu(x, pairs=False):
    """(xn, s) of the 2x2-average-pooled x in one pass (== f32_pixelnorm_silu(f32_pool2(x)), bit for bit)"""
    B, H, W, C = _nhwc32(x, "x")
    if H % 2 or W % 2 or C > 1024:
        raise ValueError("f32_pool_pixelnorm_silu: H, W even and C <= 1024 required")
    xn = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=f32)
    s = torch.empty(B, H // 2, W // 2, 2 * C, device=x.device, dtype=bf16) if pairs else torch.empty_like(xn)
    _lib.call("edm_f32_pool_pixelnorm_silu", _p(x), _p(xn), _p(s), B, H // 2, W // 2, C, int(bool(pairs)), _stream())
    return xn, s


def f32_up2_silu(x, pairs=False):
    """(y, s): y = nearest-exact x2 of x, s = mp_silu(y) as fp32 or pairs, one pass"""
    B, H, W, C = _nhwc32(x, "x")
    y = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=f32)
    s = torch.empty(B, 2 * H, 2 * W, 2 * C, device=x.device, dtype=bf16) if pairs else torch.empty_like(y)
    _lib.call("edm_f32_up2_silu", _p(x), _p(y), _p(s), B, 2 * H, 2 * W, C, int(bool(pairs)), _stream())
    return y, s


def f32_attention(qkv, heads):
    B, H, W, C3 = _nhwc32(qkv, "qkv")
    C = C3 // 3
    y = torch.empty(B, H, W, C, device=qkv.device, dtype=f32)
    N = H * W
    with _prof("f32_attention", 4.0 * B * N * N * C, 4.0 * B * N * 4 * C):
        _lib.call("edm_f32_attention", _p(qkv), _p(y), B, N, C, heads, _stream())
    return y


def split_attention_ok(C, heads, N):
    """shapes edm_split_attention covers (attention_split.hip): head_dim 64, at most 256 tokens"""
    return C % heads == 0 and C // heads == 64 and N <= 256


def split_attention(qkv, heads, pairs=False):
    """fp32-accurate attention on the bf16 matrix cores (three MFMA passes over hi/lo pairs): qkv (B,H,W,3C) fp32 in the qkv
    conv's own channel order -> (B,H,W,C) fp32, or -- pairs=True -- (B,H,W,2C) bf16 [hi | lo] pairs for the out conv"""
    B, H, W, C3 = _nhwc32(qkv, "qkv")
    C = C3 // 3
    N = H * W
    if not split_attention_ok(C, heads, N):
        raise ValueError(f"split_attention: head_dim {C // heads}, {N} tokens not covered (head_dim 64, <= 256 tokens)")
    y = torch.empty(B, H, W, 2 * C, device=qkv.device, dtype=bf16) if pairs else torch.empty(B, H, W, C, device=qkv.device, dtype=f32)
    with _prof("split_attention", 3 * 4.0 * B * N * N * C, 4.0 * B * N * 4 * C):
        _lib.call("edm_split_attention", _p(qkv), None if pairs else _p(y), _p(y) if pairs else None, B, N, C, heads, _stream())
    return y


def f32_pixelnorm_silu(x, pairs=False):
    """-> (xn fp32, s): s = mp_silu(xn) as fp32, or -- pairs=True -- as (B,H,W,2C) bf16 split pairs (split_conv's operand)"""
    B, H, W, C = _nhwc32(x, "x")
    xn = torch.empty_like(x)
    s = torch.empty(B, H, W, 2 * C, device=x.device, dtype=bf16) if pairs else torch.empty_like(x)
    _lib.call("edm_f32_pixelnorm_silu", _p(x), _p(xn), _p(s), B * H * W, C, int(bool(pairs)), _stream())
    return xn, s


def f32_silu(x, pairs=False):
    _chk(x, f32, "x")
    C = x.shape[-1]
    s = torch.empty(*x.shape[:-1], 2 * C, device=x.device, dtype=bf16) if pairs else torch.empty_like(x)
    _lib.call("edm_f32_silu", _p(x), _p(s), x.numel(), C if pairs else 0, _stream())
    return s


def f32_pool2(x):
    B, H, W, C = _nhwc32(x, "x")
    if H % 2 or W % 2:
        raise ValueError("f32_pool2: H and W must be even")
    y = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=f32)
    _lib.call("edm_f32_pool2", _p(x), _p(y), B, H // 2, W // 2, C, _stream())
    return y


def f32_up2(x):
    B, H, W, C = _nhwc32(x, "x")
    y = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=f32)
    _lib.call("edm_f32_up2", _p(x), _p(y), B, 2 * H, 2 * W, C, _stream())
    return y


def f32_skip_gate(skip, w1h, w2h):
    B, H, W, C = _nhwc32(skip, "skip")
    R = w1h.shape[0]
    _chk(w1h, f32, "w1h", (R, C + 1))
    _chk(w2h, f32, "w2h", (C, R))
    gate = torch.empty(B, C, device=skip.device, dtype=f32)
    _lib.call("edm_f32_skip_gate", _p(skip), _p(w1h), _p(w2h), _p(gate), B, H * W, C, R, _stream())
    return gate


def f32_concat_gate(inp, skip, gate, want_silu, pairs=False):
    """pairs=True: cat and sil come back as (B,H,W,2(Ci+Cs)) bf16 split pairs (they only feed convolutions)"""
    B, H, W, Ci = _nhwc32(inp, "inp")
    Bs, Hs, Ws, Cs = _nhwc32(skip, "skip")
    if (Bs, Hs, Ws) != (B, H, W):
        raise ValueError("f32_concat_gate: inp/skip spatial mismatch")
    _chk(gate, f32, "gate", (B, Cs))
    if pairs:
        cat = torch.empty(B, H, W, 2 * (Ci + Cs), device=inp.device, dtype=bf16)
    else:
        cat = torch.empty(B, H, W, Ci + Cs, device=inp.device, dtype=f32)
    sil = torch.empty_like(cat) if want_silu else None
    _lib.call("edm_f32_concat_gate", _p(inp), _p(skip), _p(gate), _p(cat), _p(sil), B, H * W, Ci, Cs, int(bool(pairs)),
              _stream())
    return cat, sil


def f32_precond_in(noisy, sigma, sigma_data, CP):
    _chk(noisy, f32, "noisy")
    B, Cimg, H, W = noisy.shape
    ss = _sigma_arg(sigma, B)
    out = torch.empty(B, H, W, CP, device=noisy.device, dtype=f32)
    _lib.call("edm_f32_precond_in", _p(noisy), _p(sigma), ss, float(sigma_data), _p(out), B, Cimg, H * W, CP, _stream())
    return out


def f32_conv_out(x, w_hat, gain_out, noisy, sigma, sigma_data):
    B, H, W, C = _nhwc32(x, "x")
    Co = w_hat.shape[0]
    _chk(w_hat, f32, "w_hat", (Co, C))
    _chk(noisy, f32, "noisy", (B, Co, H, W))
    _chk(gain_out, f32, "gain_out")
    ss = _sigma_arg(sigma, B)
    D = torch.empty(B, Co, H, W, device=x.device, dtype=f32)
    _lib.call("edm_f32_conv_out", _p(x), _p(w_hat), _p(gain_out), _p(noisy), _p(sigma), ss, float(sigma_data), _p(D), B,
              H * W, C, Co, _stream())
    return D


def f32_nchw_to_nhwc(x):
    _chk(x, f32, "x")
    B, C, H, W = x.shape
    y = torch.empty(B, H, W, C, device=x.device, dtype=f32)
    _lib.call("edm_f32_nchw_to_nhwc", _p(x), _p(y), B, C, H * W, _stream())
    return y


def f32_nhwc_to_nchw(x):
    B, H, W, C = _nhwc32(x, "x")
    y = torch.empty(B, C, H, W, device=x.device, dtype=f32)
    _lib.call("edm_f32_nhwc_to_nchw", _p(x), _p(y), B, C, H * W, _stream())
    return y


# ------------------------------------------------------------------ data formats (csrc/data.hip)
def u8_gather_normalize(data, index, mean=0.5, std=0.5, flip=False, seed=0, epoch=0):
    """data uint8 (N,C,H,W) resident on the device, index int64 (B,) -> fp32 (B,C,H,W) = (x/255-mean)/std,
    optionally flipped left-right per sample (Philox(seed; epoch, b))."""
    _chk(data, torch.uint8, "data")
    _chk(index, torch.int64, "index")
    if data.dim() != 4 or index.dim() != 1:
        raise ValueError("u8_gather_normalize: data must be (N,C,H,W), index (B,)")
    N, C, H, W = data.shape
    B = index.shape[0]
    out = torch.empty(B, C, H, W, device=data.device, dtype=f32)
    _lib.call("edm_u8_gather_normalize", _p(data), _p(index), _p(out), B, C, H, W, N, float(mean), float(std),
              int(bool(flip)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, _stream())
    return out


AUGMENT_OPS = ("xflip", "yflip", "translate", "rot90")      # bit i of the op mask; also the order they are applied in
AUGMENT_DIM = 6                                             # (xflip, yflip, sx/W, sy/H, cos(k pi/2) - 1, sin(k pi/2))


def augment_op_mask(names) -> int:
    """op names -> the 4-bit mask of edm_u8_gather_augment_normalize"""
    mask = 0
    for n in names:
        if n not in AUGMENT_OPS:
            raise ValueError(f"unknown augmentation op {n!r}: expected a subset of {AUGMENT_OPS}")
        mask |= 1 << AUGMENT_OPS.index(n)
    return mask


def u8_gather_augment_normalize(data, index, mean=0.5, std=0.5, flip=False, seed=0, epoch=0, *, p=0.0,
                                ops=AUGMENT_OPS):
    """u8_gather_normalize with the non-leaking augmentation (EDM, App. F.2; exact subset) composed into the gather ->
    (x fp32 (B,C,H,W), aug fp32 (B,6)).  Each op of `ops` is applied per sample with probability p (a 32-bit threshold,
    label_drop_threshold: p = 0 never, p = 1 always); aug holds the parameters of what was applied, zeros otherwise."""
    _chk(data, torch.uint8, "data")
    _chk(index, torch.int64, "index")
    if data.dim() != 4 or index.dim() != 1:
        raise ValueError("u8_gather_augment_normalize: data must be (N,C,H,W), index (B,)")
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"u8_gather_augment_normalize: p must be in [0, 1], got {p}")
    mask = augment_op_mask(ops) if not isinstance(ops, int) else int(ops)
    N, C, H, W = data.shape
    B = index.shape[0]
    out = torch.empty(B, C, H, W, device=data.device, dtype=f32)
    aug = torch.empty(B, AUGMENT_DIM, device=data.device, dtype=f32)
    _lib.call("edm_u8_gather_augment_normalize", _p(data), _p(index), _p(out), B, C, H, W, N, float(mean), float(std),
              int(bool(flip)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, label_drop_threshold(p), mask,
              _p(aug), _stream())
    return out, aug


AUGMENT_WARP_OPS = ("zoom", "rotate", "stretch", "shift")   # bit i of the warp mask: the continuous ops, after the exact ones
AUGMENT_DIM_WARP = 13       # AUGMENT_DIM + (n_s, cos(theta) - 1, sin(theta), n_a cos(phi), n_a sin(phi), n_x, n_y)
AUGMENT_WARP_MAX_SIZE = 64  # the resampling kernel keeps a plane and its 2x grid in LDS


def augment_warp_mask(names) -> int:
    """continuous-op names -> the 4-bit warp mask of edm_u8_gather_augment_warp_normalize"""
    mask = 0
    for n in names:
        if n not in AUGMENT_WARP_OPS:
            raise ValueError(f"unknown continuous augmentation op {n!r}: expected a subset of {AUGMENT_WARP_OPS}")
        mask |= 1 << AUGMENT_WARP_OPS.index(n)
    return mask


def u8_gather_augment_warp_normalize(data, index, mean=0.5, std=0.5, flip=False, seed=0, epoch=0, *, p=0.0,
                                     ops=AUGMENT_OPS, warp_ops=AUGMENT_WARP_OPS, return_theta=False):
    """u8_gather_augment_normalize followed by the continuous ops of the EDM pipe (zoom, rotate, stretch, shift: 2x
    upsampling, a bilinear warp, 2x downsampling; DESIGN.md, "Continuous augmentation") -> (x fp32 (B,C,H,W), aug fp32
    (B,13)), with return_theta also each sample's 2x3 matrix on the 2x grid, fp32 (B,6).  Every op of `ops` and `warp_ops`
    is applied per sample with probability p; a sample with no continuous op is u8_gather_augment_normalize's bit for bit."""
    _chk(data, torch.uint8, "data")
    _chk(index, torch.int64, "index")
    if data.dim() != 4 or index.dim() != 1:
        raise ValueError("u8_gather_augment_warp_normalize: data must be (N,C,H,W), index (B,)")
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"u8_gather_augment_warp_normalize: p must be in [0, 1], got {p}")
    mask = augment_op_mask(ops) if not isinstance(ops, int) else int(ops)
    wmask = augment_warp_mask(warp_ops) if not isinstance(warp_ops, int) else int(warp_ops)
    N, C, H, W = data.shape
    B = index.shape[0]
    out = torch.empty(B, C, H, W, device=data.device, dtype=f32)
    aug = torch.empty(B, AUGMENT_DIM_WARP, device=data.device, dtype=f32)
    theta = torch.empty(B, 6, device=data.device, dtype=f32) if return_theta else None
    _lib.call("edm_u8_gather_augment_warp_normalize", _p(data), _p(index), _p(out), B, C, H, W, N, float(mean), float(std),
              int(bool(flip)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, label_drop_threshold(p), mask,
              wmask, _p(aug), _p(theta) if return_theta else None, _stream())
    return (out, aug, theta) if return_theta else (out, aug)


def denormalize_u8(x, scale=127.5, offset=128.0):
    """fp32 tensor -> uint8, same shape: (x*scale+offset).clip(0,255) truncated."""
    _chk(x, f32, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    _lib.call("edm_denormalize_u8", _p(x), _p(out), x.numel(), float(scale), float(offset), _stream())
    return out


def prediction_to_u8_nhwc(pred, mean, std):
    """fp32 (B,C,H,W) -> uint8 (B,H,W,C): clamp(pred*std*2+mean, 0, 1)*255 truncated (per-channel mean/std tensors)."""
    _chk(pred, f32, "pred")
    B, C, H, W = pred.shape
    _chk(mean, f32, "mean", (C,))
    _chk(std, f32, "std", (C,))
    out = torch.empty(B, H, W, C, device=pred.device, dtype=torch.uint8)
    _lib.call("edm_prediction_to_u8_nhwc", _p(pred), _p(out), B, C, H, W, _p(mean), _p(std), _stream())
    return out


# ------------------------------------------------------------------ exact nearest neighbours (csrc/neighbors.hip)
KNN_MAX_K = 32
KNN_MAX_D = 32768            # 65025 * D < 2^31: every distance fits the high word of a key
KNN_MAX_SPLITS = 1024
KNN_MAX_Q = 65535 * 128      # one grid row per 128 queries
KNN_MAX_R = 2 ** 31 - 128    # row numbers of the last 128-reference tile stay 32-bit ints


def _knn_rows(t, name):
    _chk(t, torch.uint8, name)
    if t.dim() < 2 or t.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty [N, ...] tensor, got {tuple(t.shape)}")
    return t.view(t.shape[0], -1)


def knn_check(Q, R, D, k, exclude_self=False):
    """the limits of a search of Q queries against R references of D elements, as the library states them"""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"u8_knn: k must be an integer in [1, {KNN_MAX_K}], got {k!r}")
    if not 1 <= D <= KNN_MAX_D:
        raise ValueError(f"u8_knn: rows must hold 1 to {KNN_MAX_D} elements, got {D}")
    if not 1 <= Q <= KNN_MAX_Q:
        raise ValueError(f"u8_knn: expected 1 to {KNN_MAX_Q} queries, got {Q}")
    if not 1 <= R <= KNN_MAX_R:
        raise ValueError(f"u8_knn: expected 1 to 2^31 - 128 references, got {R}")
    if k > R - (1 if exclude_self else 0):
        raise ValueError(f"u8_knn: k = {k} needs at least that many references"
                         f"{' besides the query itself' if exclude_self else ''}, got R = {R}")


def u8_knn_splits(Q, R) -> int:
    """the split count of the R axis the library picks for a Q x R search"""
    return int(_lib.call("edm_u8_knn_splits", int(Q), int(R)))


def u8_knn(queries, refs, k, exclude_self=False, splits=None, *, ref_chunk=None, out=None):
    """The k nearest rows of refs (uint8 [R, ...]) for every row of queries (uint8 [Q, ...], same trailing shape; inputs of
    any rank >= 2 are taken as [N, D]) by exact squared pixel distance, ties to the lower index ->
    (dist int64 [Q, k], idx int64 [Q, k]), ascending by (dist, idx).  exclude_self: refs is the query set itself and row i
    is not its own neighbour.  splits forces the number of shares of the R axis (None: the library's plan), ref_chunk
    searches the references that many rows at a time (None: all at once); every share of every chunk leaves a sorted key
    list and one merge launch folds them, so the result depends on neither.  out=(uint32 [Q, k], int32 [Q, k]): the
    kernel's own result types are written there and returned."""
    q2, r2 = _knn_rows(queries, "queries"), _knn_rows(refs, "refs")
    if queries.shape[1:] != refs.shape[1:]:
        raise ValueError(f"u8_knn: queries {tuple(queries.shape[1:])} and refs {tuple(refs.shape[1:])} differ in shape")
    if refs.device != queries.device:
        raise ValueError(f"u8_knn: queries on {queries.device}, refs on {refs.device}")
    (Q, D), R = q2.shape, r2.shape[0]
    knn_check(Q, R, D, k, exclude_self)
    if ref_chunk is not None and (isinstance(ref_chunk, bool) or not isinstance(ref_chunk, int) or ref_chunk < 1):
        raise ValueError(f"u8_knn: ref_chunk must be None or an integer >= 1, got {ref_chunk!r}")
    chunk = R if ref_chunk is None else min(ref_chunk, R)
    bounds = [(a, min(a + chunk, R)) for a in range(0, R, chunk)]
    if splits is None:
        shares = [u8_knn_splits(Q, b - a) for a, b in bounds]
    elif isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= KNN_MAX_SPLITS:
        raise ValueError(f"u8_knn: splits must be an integer in [1, {KNN_MAX_SPLITS}], got {splits!r}")
    else:
        shares = [splits] * len(bounds)
    dev = queries.device
    if out is None:
        dist = torch.empty(Q, k, dtype=torch.uint32, device=dev)
        idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    else:
        dist, idx = out
        _chk(dist, torch.uint32, "out[0]", (Q, k))
        _chk(idx, torch.int32, "out[1]", (Q, k))
    norms = torch.empty(Q + R, dtype=torch.int32, device=dev)
    qn, rn = norms[:Q], norms[Q:]
    _lib.call("edm_u8_norms", _p(q2), Q, D, _p(qn), _stream())
    _lib.call("edm_u8_norms", _p(r2), R, D, _p(rn), _stream())
    keys = torch.empty(sum(shares), Q, k, dtype=torch.uint64, device=dev)
    at = 0
    for (a, b), s in zip(bounds, shares):
        _lib.call("edm_u8_knn_partial", _p(q2), _p(r2[a:b]), Q, b - a, D, k, int(bool(exclude_self)), a,
                  int(len(bounds) > 1), s, _p(qn), _p(rn[a:b]), _p(keys[at:at + s]), _stream())
        at += s
    _lib.call("edm_knn_merge", _p(keys), at, Q, k, _p(dist), _p(idx), _stream())
    return (dist, idx) if out is not None else (dist.to(torch.int64), idx.to(torch.int64))


def ball_radii_u32(radii, R):
    """radii: an int64 or uint32 tensor [R] with values in [0, 2^32 - 1] -> uint32 [R], contiguous (u8_ball_count's check)"""
    if not isinstance(radii, torch.Tensor) or radii.dtype not in (torch.int64, torch.uint32):
        raise ValueError(f"u8_ball_count: radii must be an int64 or uint32 tensor, got "
                         f"{radii.dtype if isinstance(radii, torch.Tensor) else type(radii).__name__}")
    if tuple(radii.shape) != (R,):
        raise ValueError(f"u8_ball_count: radii must have shape ({R},), one per reference, got {tuple(radii.shape)}")
    if radii.dtype == torch.int64:
        if bool(((radii < 0) | (radii > 0xFFFFFFFF)).any()):
            raise ValueError("u8_ball_count: radii must lie in [0, 2^32 - 1]")
        radii = radii.to(torch.uint32)          # (the low 32 bits: exact in that range)
    return radii.contiguous()


def u8_ball_count(queries, refs, radii, exclude_self=False, splits=None, *, ref_chunk=None):
    """For every row of queries (uint8 [Q, ...]) the number of rows r of refs (uint8 [R, ...], same trailing shape; inputs of
    any rank >= 2 are taken as [N, D]) whose closed ball holds it: d2(q, r) <= radii[r], d2 the exact squared pixel distance
    -> int64 [Q].  radii: int64 or uint32 [R] in [0, 2^32 - 1], one per reference.  exclude_self: refs is the query set
    itself and row i does not count for itself.  splits and ref_chunk as in u8_knn: every share of every chunk writes its
    own int32 counts and one integer sum folds them, so the result depends on neither."""
    q2, r2 = _knn_rows(queries, "queries"), _knn_rows(refs, "refs")
    if queries.shape[1:] != refs.shape[1:]:
        raise ValueError(f"u8_ball_count: queries {tuple(queries.shape[1:])} and refs {tuple(refs.shape[1:])} differ in shape")
    if refs.device != queries.device:
        raise ValueError(f"u8_ball_count: queries on {queries.device}, refs on {refs.device}")
    (Q, D), R = q2.shape, r2.shape[0]
    knn_check(Q, R, D, 1)                        # the limits on Q, R and D are those of a k = 1 search
    if not isinstance(radii, torch.Tensor) or radii.device != refs.device:
        raise ValueError(f"u8_ball_count: radii must be a tensor on {refs.device}")
    rad = ball_radii_u32(radii, R)
    if ref_chunk is not None and (isinstance(ref_chunk, bool) or not isinstance(ref_chunk, int) or ref_chunk < 1):
        raise ValueError(f"u8_ball_count: ref_chunk must be None or an integer >= 1, got {ref_chunk!r}")
    chunk = R if ref_chunk is None else min(ref_chunk, R)
    bounds = [(a, min(a + chunk, R)) for a in range(0, R, chunk)]
    if splits is None:
        shares = [u8_knn_splits(Q, b - a) for a, b in bounds]
    elif isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= KNN_MAX_SPLITS:
        raise ValueError(f"u8_ball_count: splits must be an integer in [1, {KNN_MAX_SPLITS}], got {splits!r}")
    else:
        shares = [splits] * len(bounds)
    dev = queries.device
    norms = torch.empty(Q + R, dtype=torch.int32, device=dev)
    qn, rn = norms[:Q], norms[Q:]
    _lib.call("edm_u8_norms", _p(q2), Q, D, _p(qn), _stream())
    _lib.call("edm_u8_norms", _p(r2), R, D, _p(rn), _stream())
    counts = torch.empty(sum(shares), Q, dtype=torch.int32, device=dev)
    at = 0
    for (a, b), s in zip(bounds, shares):
        _lib.call("edm_u8_ball_count_partial", _p(q2), _p(r2[a:b]), Q, b - a, D, _p(rad[a:b]), int(bool(exclude_self)), a, s,
                  _p(qn), _p(rn[a:b]), _p(counts[at:at + s]), _stream())
        at += s
    return counts.sum(0, dtype=torch.int64)


# ------------------------------------------------------------------ feature-space nearest neighbours (csrc/neighbors_f32.hip)
FKNN_MAX_Q = 65535 * 64      # one grid row per 64 queries
FKNN_MAX_R = 2 ** 31 - 64    # row numbers of the last 64-reference tile stay 32-bit ints


def _fknn_rows(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if t.dtype != f32:
        raise TypeError(f"{name}: expected float32 features, got {t.dtype} (convert with .float(); uint8 pixels go to the "
                        "u8 form)")
    if t.dim() < 2 or t.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty [N, ...] tensor, got {tuple(t.shape)}")
    _chk(t, f32, name)
    return t.view(t.shape[0], -1)


def fknn_check(Q, R, D, k, exclude_self=False):
    """the limits of a feature search of Q queries against R references of D elements, as the library states them"""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"f32_knn: k must be an integer in [1, {KNN_MAX_K}], got {k!r}")
    if not 1 <= D <= KNN_MAX_D:
        raise ValueError(f"f32_knn: rows must hold 1 to {KNN_MAX_D} elements, got {D}")
    if not 1 <= Q <= FKNN_MAX_Q:
        raise ValueError(f"f32_knn: expected 1 to {FKNN_MAX_Q} queries, got {Q}")
    if not 1 <= R <= FKNN_MAX_R:
        raise ValueError(f"f32_knn: expected 1 to 2^31 - 64 references, got {R}")
    if k > R - (1 if exclude_self else 0):
        raise ValueError(f"f32_knn: k = {k} needs at least that many references"
                         f"{' besides the query itself' if exclude_self else ''}, got R = {R}")


def f32_knn_splits(Q, R) -> int:
    """the split count of the R axis the library picks for a Q x R feature search"""
    return int(_lib.call("edm_f32_knn_splits", int(Q), int(R)))


def _fknn_plan(who, queries, refs, k, exclude_self, splits, ref_chunk):
    """the shared validation of f32_knn and f32_ball_count -> (q2, r2, chunk bounds, shares per chunk)"""
    if isinstance(queries, torch.Tensor) and isinstance(refs, torch.Tensor) and refs.device != queries.device:
        raise ValueError(f"{who}: queries on {queries.device}, refs on {refs.device}")
    q2, r2 = _fknn_rows(queries, "queries"), _fknn_rows(refs, "refs")
    if queries.shape[1:] != refs.shape[1:]:
        raise ValueError(f"{who}: queries {tuple(queries.shape[1:])} and refs {tuple(refs.shape[1:])} differ in shape")
    (Q, D), R = q2.shape, r2.shape[0]
    fknn_check(Q, R, D, k, exclude_self)
    if ref_chunk is not None and (isinstance(ref_chunk, bool) or not isinstance(ref_chunk, int) or ref_chunk < 1):
        raise ValueError(f"{who}: ref_chunk must be None or an integer >= 1, got {ref_chunk!r}")
    chunk = R if ref_chunk is None else min(ref_chunk, R)
    bounds = [(a, min(a + chunk, R)) for a in range(0, R, chunk)]
    if splits is None:
        shares = [f32_knn_splits(Q, b - a) for a, b in bounds]
    elif isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= KNN_MAX_SPLITS:
        raise ValueError(f"{who}: splits must be an integer in [1, {KNN_MAX_SPLITS}], got {splits!r}")
    else:
        shares = [splits] * len(bounds)
    return q2, r2, bounds, shares


def f32_norms(x):
    """fp64 [N]: |x|^2 of the rows of a float32 [N, ...] tensor with the bits of the distance tile's x . x (edm_f32_norms), so
    that identical rows are at distance +0.0 exactly"""
    x2 = _fknn_rows(x, "x")
    if not 1 <= x2.shape[1] <= KNN_MAX_D or x2.shape[0] > FKNN_MAX_R:
        raise ValueError(f"f32_norms: expected at most 2^31 - 64 rows of 1 to {KNN_MAX_D} elements, got {tuple(x2.shape)}")
    out = torch.empty(x2.shape[0], dtype=torch.float64, device=x.device)
    _lib.call("edm_f32_norms", _p(x2), x2.shape[0], x2.shape[1], _p(out), _stream())
    return out


def _fknn_norms(q2, r2):
    """the norms of both sets (one launch when the references are the queries)"""
    qn = f32_norms(q2)
    same = q2.data_ptr() == r2.data_ptr() and q2.shape == r2.shape
    return qn, (qn if same else f32_norms(r2))


def f32_knn(queries, refs, k, exclude_self=False, splits=None, *, ref_chunk=None):
    """The k nearest rows of refs (float32 [R, ...]) for every row of queries (float32 [Q, ...], same trailing shape; inputs
    of any rank >= 2 are taken as [N, D]) by squared Euclidean distance in fp64, d2 = max(|q|^2 + |r|^2 - 2 q.r, 0), ties to
    the lower index -> (dist fp64 [Q, k], idx int64 [Q, k]), ascending by (dist, idx).  exclude_self, splits and ref_chunk as
    in u8_knn; the bits of a distance depend on the two rows only, so the result depends on neither splits nor ref_chunk.
    The input must be finite (the callers that take a set in check it once; nothing is scanned per call)."""
    q2, r2, bounds, shares = _fknn_plan("f32_knn", queries, refs, k, exclude_self, splits, ref_chunk)
    (Q, D), dev = q2.shape, queries.device
    qn, rn = _fknn_norms(q2, r2)
    n = sum(shares)
    keys_d2 = torch.empty(n, Q, k, dtype=torch.uint64, device=dev)
    keys_idx = torch.empty(n, Q, k, dtype=torch.int32, device=dev)
    at = 0
    for (a, b), s in zip(bounds, shares):
        _lib.call("edm_f32_knn_partial", _p(q2), _p(r2[a:b]), Q, b - a, D, k, int(bool(exclude_self)), a,
                  int(len(bounds) > 1), s, _p(qn), _p(rn[a:b]), _p(keys_d2[at:at + s]), _p(keys_idx[at:at + s]), _stream())
        at += s
    dist = torch.empty(Q, k, dtype=torch.float64, device=dev)
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    _lib.call("edm_fknn_merge", _p(keys_d2), _p(keys_idx), at, Q, k, _p(dist), _p(idx), _stream())
    return dist, idx.to(torch.int64)


def ball_radii_f64(radii, R):
    """radii: an fp64 tensor [R], finite and >= 0 -> contiguous (f32_ball_count's check)"""
    if not isinstance(radii, torch.Tensor) or radii.dtype != torch.float64:
        raise ValueError(f"f32_ball_count: radii must be a float64 tensor, got "
                         f"{radii.dtype if isinstance(radii, torch.Tensor) else type(radii).__name__}")
    if tuple(radii.shape) != (R,):
        raise ValueError(f"f32_ball_count: radii must have shape ({R},), one per reference, got {tuple(radii.shape)}")
    if not bool((torch.isfinite(radii) & (radii >= 0)).all()):
        raise ValueError("f32_ball_count: radii must be finite and >= 0")
    return radii.contiguous()


def f32_ball_count(queries, refs, radii, exclude_self=False, splits=None, *, ref_chunk=None):
    """For every row of queries (float32 [Q, ...]) the number of rows r of refs (float32 [R, ...], same trailing shape) whose
    closed ball holds it: d2(q, r) <= radii[r], d2 as in f32_knn (the same bits: a radius taken from f32_knn is compared
    with the very number it was) -> int64 [Q].  radii: fp64 [R], finite and >= 0.  exclude_self, splits and ref_chunk as in
    u8_ball_count: every share of every chunk writes its own int32 counts and one integer sum folds them."""
    q2, r2, bounds, shares = _fknn_plan("f32_ball_count", queries, refs, 1, False, splits, ref_chunk)
    (Q, D), R, dev = q2.shape, r2.shape[0], queries.device
    if not isinstance(radii, torch.Tensor) or radii.device != refs.device:
        raise ValueError(f"f32_ball_count: radii must be a tensor on {refs.device}")
    rad = ball_radii_f64(radii, R)
    qn, rn = _fknn_norms(q2, r2)
    counts = torch.empty(sum(shares), Q, dtype=torch.int32, device=dev)
    at = 0
    for (a, b), s in zip(bounds, shares):
        _lib.call("edm_f32_ball_count_partial", _p(q2), _p(r2[a:b]), Q, b - a, D, _p(rad[a:b]), int(bool(exclude_self)), a, s,
                  _p(qn), _p(rn[a:b]), _p(counts[at:at + s]), _stream())
        at += s
    return counts.sum(0, dtype=torch.int64)


# ------------------------------------------------------------------ ideal denoiser of a training set (csrc/ideal.hip)
IDEAL_MAX_K = 32768              # elements per image (edm_u8_norms' limit: |u - 128|^2 summed in an int)
IDEAL_MAX_Q = 65535 * 64         # one grid row per 64 queries
IDEAL_MAX_R = 2 ** 31 - 128      # reference indices are 32-bit ints
IDEAL_REF_CHUNK = 8192           # default rows per chunk: the workspace is Q * chunk floats
IDEAL_STATE = 8                  # floats of running state per query


def ideal_check(Q, R, K, ref_chunk=None):
    """the limits of an ideal-denoiser call of Q queries against R references of K elements, as the library states them
    -> the chunk length"""
    if not 1 <= K <= IDEAL_MAX_K:
        raise ValueError(f"ideal_denoise: images must hold 1 to {IDEAL_MAX_K} elements, got {K}")
    if not 1 <= Q <= IDEAL_MAX_Q:
        raise ValueError(f"ideal_denoise: expected 1 to {IDEAL_MAX_Q} queries, got {Q}")
    if not 1 <= R <= IDEAL_MAX_R:
        raise ValueError(f"ideal_denoise: expected 1 to 2^31 - 128 references, got {R}")
    if ref_chunk is not None and (isinstance(ref_chunk, bool) or not isinstance(ref_chunk, int) or ref_chunk < 1):
        raise ValueError(f"ideal_denoise: ref_chunk must be None or an integer >= 1, got {ref_chunk!r}")
    return min(IDEAL_REF_CHUNK if ref_chunk is None else ref_chunk, R)


def ideal_norm_check(mean, std):
    mean, std = float(mean), float(std)
    if not (math.isfinite(mean) and math.isfinite(std) and std > 0.0):
        raise ValueError(f"ideal_denoise: mean must be finite and std finite and > 0, got {mean}, {std}")
    return mean, std


def u8_norms(x):
    """int32 [N]: sum_j (x_j - 128)^2 of the rows of a uint8 [N, ...] tensor (edm_u8_norms)"""
    x2 = _knn_rows(x, "x")
    if not 1 <= x2.shape[1] <= KNN_MAX_D or x2.shape[0] > KNN_MAX_R:
        raise ValueError(f"u8_norms: expected at most 2^31 - 128 rows of 1 to {KNN_MAX_D} elements, got {tuple(x2.shape)}")
    out = torch.empty(x2.shape[0], dtype=torch.int32, device=x.device)
    _lib.call("edm_u8_norms", _p(x2), x2.shape[0], x2.shape[1], _p(out), _stream())
    return out


def ideal_denoise(x, sigma, refs, rnorms, mean=0.5, std=0.5, *, ref_labels=None, labels=None, num_classes=None,
                  ref_chunk=None):
    """The ideal denoiser D*(x; sigma) of the uint8 set `refs` (y = (u / 255 - mean) / std) and its statistics ->
    (D fp32 like x, lse fp32 [Q], ent fp32 [Q], top_w fp32 [Q], top_idx int32 [Q]).  x: contiguous fp32 [Q, ...] with the
    trailing shape of refs (uint8 [R, ...], contiguous, any byte alignment); sigma: fp32 [Q]; rnorms: int32 [R], u8_norms
    of refs.  ref_labels (int32 [R]) with labels (int64 [Q]) and num_classes restrict the softmax of query q to the
    references of class labels[q]; labels=None uses every reference.  The references are walked ref_chunk rows at a time
    (None: 8192) with a Q x ref_chunk workspace.  A sigma <= 0 or non-finite, a non-finite x row or a label outside
    [0, num_classes) gives that row NaN (top_idx -1) and sets the health bit (check_health)."""
    _chk_eval(x, f32, "x")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"x: expected a non-empty [Q, ...] tensor, got {tuple(x.shape)}")
    dev = x.device
    _chk_eval(refs, torch.uint8, "refs", None, dev)
    if refs.dim() < 2 or refs.numel() == 0 or tuple(refs.shape[1:]) != tuple(x.shape[1:]):
        raise ValueError(f"ideal_denoise: refs {tuple(refs.shape)} must be a non-empty [R, ...] set of x's image shape "
                         f"{tuple(x.shape[1:])}")
    Q, R = x.shape[0], refs.shape[0]
    K = x.numel() // Q
    chunk = ideal_check(Q, R, K, ref_chunk)
    mean, std = ideal_norm_check(mean, std)
    _chk_eval(sigma, f32, "sigma", (Q,), dev)
    _chk_eval(rnorms, torch.int32, "rnorms", (R,), dev)
    ncls = 0
    if labels is not None:
        if ref_labels is None:
            raise ValueError("ideal_denoise: labels need ref_labels (the classes of the references)")
        ncls = _chk_classes(num_classes)
        if ncls >= 1 << 31:
            raise ValueError(f"ideal_denoise: num_classes must be below 2**31, got {ncls}")
        _chk_eval(labels, torch.int64, "labels", (Q,), dev)
    if ref_labels is not None:
        _chk_eval(ref_labels, torch.int32, "ref_labels", (R,), dev)
    r2 = refs.view(R, K)
    ld = (chunk + 3) // 4 * 4
    S = torch.empty(Q, ld, dtype=f32, device=dev)
    qd = torch.empty(Q, 2, dtype=torch.float64, device=dev)
    state = torch.empty(Q, IDEAL_STATE, dtype=f32, device=dev)
    D = torch.empty_like(x)
    lse, ent, top_w = (torch.empty(Q, dtype=f32, device=dev) for _ in range(3))
    top_idx = torch.empty(Q, dtype=torch.int32, device=dev)
    hw, st = _p(health(dev)), _stream()
    masked = labels is not None
    _lib.call("edm_ideal_begin", _p(x), _p(sigma), _p(labels), ncls, Q, K, mean, std, _p(qd), _p(state), hw, st)
    with _prof("ideal", 4.0 * Q * R * K, float(R) * K * 2 * ((Q + 63) // 64)):
        for a in range(0, R, chunk):
            n = min(chunk, R - a)
            _lib.call("edm_ideal_logits", _p(x), _p(r2[a:a + n]), _p(rnorms[a:a + n]), _p(qd), Q, n, K, mean, std, _p(S),
                      ld, st)
            _lib.call("edm_ideal_softmax", _p(S), ld, Q, n, a, _p(ref_labels) if masked else None,
                      _p(labels) if masked else None, _p(state), st)
            _lib.call("edm_ideal_accumulate", _p(S), ld, _p(r2[a:a + n]), _p(state), Q, n, K, int(a == 0), _p(D), st)
    _lib.call("edm_ideal_finish", _p(D), _p(state), Q, K, mean, std, _p(D), _p(lse), _p(ent), _p(top_w), _p(top_idx), hw, st)
    return D, lse, ent, top_w, top_idx


# ------------------------------------------------------------------ fp64 moments and polynomial-kernel sums (csrc/moments.hip)
MOMENTS_MAX_D = 32768
MOMENTS_MAX_SPLITS = 1024
POLY_MAX_M = 65535 * 64          # one grid row / column per 64 rows of a subset
POLY_MAX_S = 65535
POLY_MAX_D = 2 ** 24


def _f64_rows(t, name):
    """a set for the fp64 reductions: uint8 or float32 [n, ...] on the device, contiguous -> (the [n, D] view, dtype code)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if t.dtype not in (torch.uint8, f32):
        raise TypeError(f"{name}: expected uint8 pixels or float32 features, got {t.dtype} (convert features with .float())")
    if t.dim() < 2 or t.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty [n, ...] tensor (D >= 1), got {tuple(t.shape)}")
    _chk(t, t.dtype, name)
    return t.view(t.shape[0], -1), 0 if t.dtype == torch.uint8 else 1


def _row_index(index, rows, name, dev, dims):
    """an int64 index tensor of `dims` dimensions on `dev`, every entry a row number in [0, rows)"""
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != dims or index.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty int64 tensor of {dims} dimension(s), got "
                         f"{(index.dtype, tuple(index.shape)) if isinstance(index, torch.Tensor) else type(index).__name__}")
    _chk_eval(index, torch.int64, name, None, dev)
    lo, hi = int(index.min()), int(index.max())
    if lo < 0 or hi >= rows:
        raise ValueError(f"{name}: entries must lie in [0, {rows}), got {lo} .. {hi}")
    return index


def moments_splits(N, D) -> int:
    """the number of shares of the N axis the library picks for the moments of an N x D set"""
    return int(_lib.call("edm_moments_splits", int(N), int(D)))


def moments(x, index=None, shift=None, splits=None, *, sums_only=False):
    """(sum fp64 [D], gram fp64 [D, D]) of the rows of x (uint8 or float32 [n, ...], taken as [n, D]): sum = sum_i y_i and
    gram = sum_i y_i y_i^T with y_i = x[index[i]] - shift in fp64.  index: int64 [N] on the device, any order, repeats
    allowed (None: every row once).  shift: fp64 [D] on the device (None: 0).  uint8 rows without a shift give exact
    integers, whatever `splits` (the number of shares of the N axis; None: the library's plan); float32 rows give the same
    bits for the same arguments.  sums_only: the column sums alone, (sum, None)."""
    x2, code = _f64_rows(x, "x")
    D = x2.shape[1]
    if D > MOMENTS_MAX_D:
        raise ValueError(f"moments: rows must hold 1 to {MOMENTS_MAX_D} elements, got {D}")
    if splits is not None and (isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= MOMENTS_MAX_SPLITS):
        raise ValueError(f"moments: splits must be None or an integer in [1, {MOMENTS_MAX_SPLITS}], got {splits!r}")
    dev = x.device
    if index is not None:
        _row_index(index, x2.shape[0], "index", dev, 1)
    if shift is not None:
        _chk_eval(shift, torch.float64, "shift", (D,), dev)
    N = x2.shape[0] if index is None else index.shape[0]
    S = moments_splits(N, D) if splits is None else splits
    psum = torch.empty(S, D, dtype=torch.float64, device=dev)
    pgram = None if sums_only else torch.empty(S, D, D, dtype=torch.float64, device=dev)
    out_sum = torch.empty(D, dtype=torch.float64, device=dev)
    gram = None if sums_only else torch.empty(D, D, dtype=torch.float64, device=dev)
    with _prof("moments", 0.0 if sums_only else 2.0 * N * D * D, float(N) * D * x.element_size()):
        _lib.call("edm_moments_partial", _p(x2), code, _p(index), N, D, _p(shift), S, _p(psum), _p(pgram), _stream())
        _lib.call("edm_moments_finish", _p(psum), _p(pgram), S, D, _p(out_sum), _p(gram), _stream())
    return out_sum, gram


def poly_kernel_sums(a, idx_a, b, idx_b, gamma, coef0, degree, exclude_equal_index=False):
    """sums fp64 [S]: for each subset s the sum over i < ma, j < mb of (gamma a[idx_a[s, i]] . b[idx_b[s, j]] + coef0)^degree
    in fp64.  a, b: uint8 or float32 [n, ...] with the same number of elements per row (taken as [n, D]); idx_a int64
    [S, ma], idx_b int64 [S, mb] on the device (None: every row of the set in order, as one subset).  degree: 1 to 4.
    exclude_equal_index skips the pairs with idx_a[s, i] == idx_b[s, j] (the diagonal of a set against itself; by index, so
    a duplicate row still counts).  Same arguments, same bits."""
    if isinstance(degree, bool) or not isinstance(degree, int) or not 1 <= degree <= 4:
        raise ValueError(f"poly_kernel_sums: degree must be an integer in [1, 4], got {degree!r}")
    gamma, coef0 = float(gamma), float(coef0)
    if not (math.isfinite(gamma) and math.isfinite(coef0)):
        raise ValueError(f"poly_kernel_sums: gamma and coef0 must be finite, got {gamma}, {coef0}")
    a2, code_a = _f64_rows(a, "a")
    b2, code_b = _f64_rows(b, "b")
    D = a2.shape[1]
    if b2.shape[1] != D:
        raise ValueError(f"poly_kernel_sums: rows of a hold {D} elements, rows of b {b2.shape[1]}")
    if D > POLY_MAX_D:
        raise ValueError(f"poly_kernel_sums: rows must hold 1 to {POLY_MAX_D} elements, got {D}")
    dev = a.device
    if b.device != dev:
        raise ValueError(f"poly_kernel_sums: a on {dev}, b on {b.device}")
    if idx_a is not None:
        _row_index(idx_a, a2.shape[0], "idx_a", dev, 2)
    if idx_b is not None:
        _row_index(idx_b, b2.shape[0], "idx_b", dev, 2)
    S = 1 if idx_a is None else idx_a.shape[0]
    if (1 if idx_b is None else idx_b.shape[0]) != S:
        raise ValueError(f"poly_kernel_sums: idx_a and idx_b must list the same number of subsets (None counts as one)")
    ma = a2.shape[0] if idx_a is None else idx_a.shape[1]
    mb = b2.shape[0] if idx_b is None else idx_b.shape[1]
    if not 1 <= S <= POLY_MAX_S or ma > POLY_MAX_M or mb > POLY_MAX_M:
        raise ValueError(f"poly_kernel_sums: expected 1 to {POLY_MAX_S} subsets of at most {POLY_MAX_M} rows, got {S} of "
                         f"{ma} x {mb}")
    tiles = ((ma + 63) // 64) * ((mb + 63) // 64)
    partial = torch.empty(S, tiles, dtype=torch.float64, device=dev)
    sums = torch.empty(S, dtype=torch.float64, device=dev)
    with _prof("poly_kernel_sums", 2.0 * S * ma * mb * D, float(S) * (ma + mb) * D * a.element_size()):
        _lib.call("edm_poly_sums_partial", _p(a2), code_a, _p(idx_a), _p(b2), code_b, _p(idx_b), S, ma, mb, D, gamma, coef0,
                  degree, int(bool(exclude_equal_index)), _p(partial), _stream())
        _lib.call("edm_poly_sums_finish", _p(partial), S, tiles, _p(sums), _stream())
    return sums


# ------------------------------------------------------------------ denoiser activations as features (csrc/features.hip)
def f32_pool_features(x, out=None, offset=0):
    """The spatial mean of an fp32 NHWC activation (B,H,W,C) as feature columns: out[b, offset + c] = the mean over H*W of
    x[b, :, :, c], summed in fp64 in an order that depends on H*W alone and rounded to fp32 once -- row b has the same bits
    whatever the batch.  out=None allocates and returns (B, C); otherwise out is a contiguous fp32 (B, Dtot) tensor with
    offset + C <= Dtot, only those C columns are written, and out is returned.  Any C >= 1, any B."""
    try:
        B, H, W, C = _nhwc32(x, "x")
    except (TypeError, RuntimeError) as e:
        raise ValueError(str(e)) from None
    if x.numel() == 0:
        raise ValueError(f"x: expected a non-empty (B,H,W,C) tensor, got {tuple(x.shape)}")
    if isinstance(offset, bool) or not isinstance(offset, int) or offset < 0:
        raise ValueError(f"f32_pool_features: offset must be an integer >= 0, got {offset!r}")
    if out is None:
        if offset:
            raise ValueError("f32_pool_features: an offset needs the out tensor it points into")
        out = torch.empty(B, C, device=x.device, dtype=f32)
    else:
        _chk_eval(out, f32, "out", None, x.device)
        if out.dim() != 2 or out.shape[0] != B or offset + C > out.shape[1]:
            raise ValueError(f"out: expected ({B}, Dtot) with Dtot >= offset + C = {offset + C}, got {tuple(out.shape)}")
    with _prof("f32_pool_features", 0.0, 4.0 * (x.numel() + B * C)):
        _lib.call("edm_f32_pool_features", _p(x), _p(out), B, H * W, C, out.shape[1], offset, _stream())
    return out


# ------------------------------------------------------------------ feature clustering (csrc/kmeans.hip)
CLUSTER_MAX_K = 2 ** 20


def cluster_block() -> int:
    """EDM_CLUSTER_BLOCK as the loaded library was built: rows per chunk of a cluster's member list (the chunk tables are
    cut with the library's own value, so a library built with another chunk length gets tables that fit it)"""
    return int(_lib.call("edm_cluster_block"))


def _cluster_index(labels, K, counts):
    """the inverted index of int64 labels [n] in [0, K) -> (members int32 [n], starts int32 [K + 1], chunk_first int32
    [K + 1], chunk_cluster int32 [chunks]): cluster k's rows in ascending row number (a stable sort), cut into chunks of
    cluster_block() rows.  counts: the bincount of the labels as a numpy int64 [K] array; the tables are made from it on
    the host (K entries), so nothing here waits for the device."""
    dev, block = labels.device, cluster_block()
    members = torch.sort(labels, stable=True).indices.to(torch.int32)
    per = (counts + (block - 1)) // block
    starts, first = np.zeros(K + 1, np.int64), np.zeros(K + 1, np.int64)
    np.cumsum(counts, out=starts[1:])
    np.cumsum(per, out=first[1:])
    chunk_cluster = np.repeat(np.arange(K, dtype=np.int32), per)
    up = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)       # noqa: E731
    return members, up(starts), up(first), up(chunk_cluster)


def f32_cluster_sums(x, labels, K, d2=None, *, counts=None):
    """Per-cluster sums of the rows of x (float32 [n, ...], taken as [n, D]) -> (sums fp64 [K, D], counts int64 [K], d2sums
    fp64 [K] or None): sums[k] = the fp64 column sums of the rows with labels == k, each float32 widened as it is loaded,
    and d2sums[k] = the sum of d2 (fp64 [n] or None) over the same rows.  labels: int64 [n] on the device, any order, every
    entry in [0, K).  The addition order is a function of a cluster's member list alone (ascending row number, chunks of
    cluster_block() rows added in order: include/tinyedm_hip.h), so the same arguments give the same bits and the sums of
    a cluster do not depend on K or on the other clusters.  No atomics and no fp64 copy of the set: the workspace is at
    most (n / cluster_block() + K)(D + 1) doubles.  An empty cluster gives +0.0 and a count of 0.  The input must be finite
    (the callers that take a set in check it once).
    The call waits for the device three times (the least and the largest label, then the counts, from which the chunk
    tables are made on the host).  counts: the bincount of the labels as a numpy int64 [K] array, from a caller that made
    the labels itself and holds it already (cluster.lloyd_step): the labels are then taken as valid and the call reads
    nothing back.  Counts that do not belong to the labels give wrong sums, never an access outside the set."""
    x2 = _fknn_rows(x, "x")
    n, D = x2.shape
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= CLUSTER_MAX_K:
        raise ValueError(f"f32_cluster_sums: K must be an integer in [1, {CLUSTER_MAX_K}], got {K!r}")
    if not 1 <= D <= KNN_MAX_D or n > FKNN_MAX_R:
        raise ValueError(f"f32_cluster_sums: expected at most 2^31 - 64 rows of 1 to {KNN_MAX_D} elements, got {tuple(x2.shape)}")
    dev = x.device
    if counts is None:
        _row_index(labels, K, "labels", dev, 1)
    else:
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() != 1:
            raise ValueError("labels: expected an int64 tensor of 1 dimension")
        _chk_eval(labels, torch.int64, "labels", None, dev)
        if not (isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.shape == (K,)
                and int(counts.min()) >= 0 and int(counts.sum()) == n):
            raise ValueError(f"counts: expected a numpy int64 [{K}] array of non-negative counts that add up to {n}")
    if labels.shape[0] != n:
        raise ValueError(f"labels: expected one label per row ({n}), got {labels.shape[0]}")
    if d2 is not None:
        _chk_eval(d2, torch.float64, "d2", (n,), dev)
    if counts is None:
        counts_dev = torch.bincount(labels, minlength=K)
        counts = counts_dev.cpu().numpy()
    else:
        counts_dev = torch.from_numpy(counts).to(dev)
    members, starts, first, chunk_cluster = _cluster_index(labels, K, counts)
    chunks = chunk_cluster.shape[0]
    partial = torch.empty(chunks, D, dtype=torch.float64, device=dev)
    partial_d2 = None if d2 is None else torch.empty(chunks, dtype=torch.float64, device=dev)
    sums = torch.empty(K, D, dtype=torch.float64, device=dev)
    d2sums = None if d2 is None else torch.empty(K, dtype=torch.float64, device=dev)
    with _prof("f32_cluster_sums", float(n) * D, 4.0 * n * D + 16.0 * chunks * D + 8.0 * K * D):
        _lib.call("edm_f32_cluster_sums_partial", _p(x2), _p(members), _p(starts), _p(first), _p(chunk_cluster), _p(d2), n, D,
                  K, chunks, _p(partial), _p(partial_d2), _stream())
        _lib.call("edm_f32_cluster_sums_finish", _p(partial), _p(partial_d2), _p(first), D, K, _p(sums), _p(d2sums), _stream())
    return sums, counts_dev, d2sums


# ------------------------------------------------------------------ optimised sampling schedules (csrc/schedule.hip)
SCHEDULE_MAX_GRID = 256         # EDM_SCHEDULE_MAX_GRID: nodes of the teacher grid edm_pair_step_errors takes


def pair_step_errors(X, S, tau, order=2):
    """The squared local error of every single-step jump i -> j between the nodes of a recorded trajectory
    (DeterministicSolver.trace): X fp32 [G + 1, B, ...] the states, S fp32 [G, B, ...] the Euler slopes, tau fp64 [G + 1]
    on the device (the table widened, tau[G] = 0).  Returns d2 fp64 [B, G, G + 1]; for i < j, in fp64,

        d2[b, i, j] = sum_k (x_i + h s_i - x_j)^2                (order 1, and order 2 when j == G),   h = tau[j] - tau[i]
        d2[b, i, j] = sum_k (x_i + h/2 (s_i + s_j) - x_j)^2      (order 2, j < G: the trapezoid along the trajectory)

    and +0.0 where j <= i.  The bits of an entry depend on K, the two nodes' rows of the sample, tau[i], tau[j] and order
    alone (include/tinyedm_hip.h).  1 <= G <= SCHEDULE_MAX_GRID."""
    _chk_eval(X, f32, "X")
    if X.dim() < 3 or X.numel() == 0 or X.shape[0] < 2:
        raise ValueError(f"X: expected a non-empty fp32 [G + 1, B, ...] tensor with G >= 1, got {tuple(X.shape)}")
    G, B = X.shape[0] - 1, X.shape[1]
    if G > SCHEDULE_MAX_GRID:
        raise ValueError(f"pair_step_errors: at most {SCHEDULE_MAX_GRID} grid nodes, got {G}")
    _chk_eval(S, f32, "S", (G, *X.shape[1:]), X.device)
    _chk_eval(tau, torch.float64, "tau", (G + 1,), X.device)
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"pair_step_errors: order must be 1 (Euler) or 2 (trapezoid), got {order!r}")
    K = X.numel() // ((G + 1) * B)
    d2 = torch.empty((B, G, G + 1), dtype=torch.float64, device=X.device)
    pairs = B * G * (G + 1) // 2
    with _prof("pair_step_errors", 6.0 * pairs * K, 4.0 * (X.numel() + S.numel()) + 8.0 * d2.numel()):
        _lib.call("edm_pair_step_errors", _p(X), _p(S), _p(tau), B, G, K, int(order), _p(d2), _stream())
    return d2


# ------------------------------------------------------------------ paired image quality (csrc/quality.hip)
SSIM_MAX_WIN = 15               # the widest window edm_pair_ssim takes
FEATURE_DISTANCE_MAX_C = 768    # channels of a pixel row edm_f32_pair_feature_distance keeps in one wave's registers


def _ssim_window(window):
    """the host-built fp64 tap table -> a numpy fp64 [win] array (checked)"""
    if isinstance(window, torch.Tensor):
        if window.is_cuda:
            raise ValueError("pair_ssim: window is the HOST-built tap table (numpy or a CPU tensor), not a device tensor")
        window = window.numpy()
    w = np.asarray(window)
    if w.dtype != np.float64 or w.ndim != 1:
        raise ValueError(f"pair_ssim: window must be a 1-d fp64 table, got {w.dtype} {w.shape}")
    win = w.shape[0]
    if win % 2 == 0 or not 3 <= win <= SSIM_MAX_WIN:
        raise ValueError(f"pair_ssim: the window must have an odd number of taps in [3, {SSIM_MAX_WIN}], got {win}")
    if not np.isfinite(w).all():
        raise ValueError("pair_ssim: window holds non-finite taps")
    return np.ascontiguousarray(w)


def pair_ssim(a, b, window, data_range, region=None):
    """SSIM and the squared error of image i of a against image i of b -> (ssim fp64 [n, C], sse fp64 [n, C], counts int32
    [n, 2]).  a, b: the same shape and dtype, uint8 [n, H, W, C] (the PNG layout) or float32 [n, C, H, W] in pixel units,
    any non-negative strides (the kernel takes element strides: no copy to a common layout).  window: the fp64 1-D tap
    table built on the host (compare.gaussian_window / uniform_window), odd, 3 <= win <= 15, win <= min(H, W).
    data_range L: C1 = (0.01 L)^2, C2 = (0.03 L)^2; uint8 takes 255.  Everything is fp64 over the valid region (no
    padding), biased variances.  sse = sum (a - b)^2 over the counted pixels (uint8: an exact integer).  region: uint8
    [n or 1, H, W], non-zero = counted: sse over counted pixels, the SSIM mean over valid centres that are themselves
    counted; counts = (counted pixels, counted centres); no counted centre gives NaN and a count of 0.  The bits of row i
    depend on that pair, the shape, the window and the region row alone (include/tinyedm_hip.h)."""
    for t, name in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name}: expected a CUDA/HIP tensor -- tinyedm_amd has no CPU path")
    if a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
        raise ValueError(f"pair_ssim: a and b must agree in dtype, shape and device, got {a.dtype} {tuple(a.shape)} on "
                         f"{a.device} and {b.dtype} {tuple(b.shape)} on {b.device}")
    if a.dtype not in (torch.uint8, f32) or a.dim() != 4 or a.numel() == 0:
        raise ValueError(f"pair_ssim: expected non-empty uint8 [n, H, W, C] or float32 [n, C, H, W] images, got {a.dtype} "
                         f"{tuple(a.shape)}")
    is_u8 = a.dtype == torch.uint8
    if is_u8:
        n, H, W, C = a.shape
        order = (0, 3, 1, 2)
    else:
        n, C, H, W = a.shape
        order = (0, 1, 2, 3)
    w = _ssim_window(window)
    win = w.shape[0]
    if win > min(H, W):
        raise ValueError(f"pair_ssim: a window of {win} taps does not fit {H} x {W} images")
    try:
        L = float(data_range)
    except (TypeError, ValueError):
        raise ValueError(f"pair_ssim: data_range must be a number, got {data_range!r}") from None
    if not (math.isfinite(L) and L > 0.0):
        raise ValueError(f"pair_ssim: data_range must be finite and > 0, got {data_range}")
    if is_u8 and L != 255.0:
        raise ValueError(f"pair_ssim: uint8 images have data_range 255, got {data_range}")
    sa, sb = [a.stride(k) for k in order], [b.stride(k) for k in order]
    if min(sa) < 0 or min(sb) < 0:
        raise ValueError("pair_ssim: negative strides")
    dev = a.device
    shared = 0
    if region is not None:
        _chk_eval(region, torch.uint8, "region", None, dev)
        if region.dim() != 3 or region.shape[0] not in (1, n) or tuple(region.shape[1:]) != (H, W):
            raise ValueError(f"region: expected uint8 [{n} or 1, {H}, {W}], got {tuple(region.shape)}")
        shared = int(region.shape[0] == 1 and n > 1)
    tiles = int(_lib.call("edm_pair_ssim_tiles", H, W, win))
    if tiles < 1 or H * W >= 2 ** 31 or n * C * tiles >= 2 ** 31:
        raise ValueError(f"pair_ssim: {n} x {C} planes of {H} x {W} exceed the library's limits")
    wdev = torch.from_numpy(w).to(dev)
    partial = torch.empty(n * C * tiles, 4, dtype=torch.float64, device=dev)
    ssim = torch.empty(n, C, dtype=torch.float64, device=dev)
    sse = torch.empty(n, C, dtype=torch.float64, device=dev)
    counts = torch.empty(n, 2, dtype=torch.int32, device=dev)
    with _prof("pair_ssim", 20.0 * win * n * C * H * W, 2.0 * a.element_size() * n * C * H * W):
        _lib.call("edm_pair_ssim", _p(a), _p(b), int(is_u8), n, C, H, W, (ctypes.c_long * 4)(*sa), (ctypes.c_long * 4)(*sb),
                  _p(wdev), win, L, _p(region), shared, _p(partial), _p(ssim), _p(sse), _p(counts), _stream())
    return ssim, sse, counts


def f32_pair_feature_distance(a, b, out=None, column=0):
    """The LPIPS form of a distance between two sets of fp32 NHWC maps (B,H,W,C) of one tap -> fp64:
    d[b] = (1/HW) sum_p sum_c (a_pc / (|a_p| + 1e-10) - b_pc / (|b_p| + 1e-10))^2, two passes per pixel (the norms, then
    the squared differences of the scaled values), summed in fp64 in an order fixed by (HW, C): row b has the same bits
    whatever the batch, identical inputs give exactly 0.0, an all-zero pixel stays finite.  out=None allocates and
    returns fp64 (B,); otherwise out is a contiguous fp64 (B, T) tensor, only column `column` is written and out is
    returned, so several taps sit side by side.  1 <= C <= FEATURE_DISTANCE_MAX_C."""
    try:
        B, H, W, C = _nhwc32(a, "a")
        _nhwc32(b, "b")
    except (TypeError, RuntimeError) as e:
        raise ValueError(str(e)) from None
    if a.numel() == 0 or a.shape != b.shape or a.device != b.device:
        raise ValueError(f"f32_pair_feature_distance: expected two non-empty (B,H,W,C) maps of one shape on one device, got "
                         f"{tuple(a.shape)} and {tuple(b.shape)}")
    if C > FEATURE_DISTANCE_MAX_C:
        raise ValueError(f"f32_pair_feature_distance: at most {FEATURE_DISTANCE_MAX_C} channels, got {C}")
    if isinstance(column, bool) or not isinstance(column, int) or column < 0:
        raise ValueError(f"f32_pair_feature_distance: column must be an integer >= 0, got {column!r}")
    if out is None:
        if column:
            raise ValueError("f32_pair_feature_distance: a column needs the out tensor it points into")
        res = torch.empty(B, 1, device=a.device, dtype=torch.float64)
    else:
        _chk_eval(out, torch.float64, "out", None, a.device)
        if out.dim() != 2 or out.shape[0] != B or column >= out.shape[1]:
            raise ValueError(f"out: expected ({B}, T) with T > column = {column}, got {tuple(out.shape)}")
        res = out
    with _prof("f32_pair_feature_distance", 8.0 * a.numel(), 8.0 * a.numel()):
        _lib.call("edm_f32_pair_feature_distance", _p(a), _p(b), _p(res), B, H * W, C, res.shape[1], column, _stream())
    return res.view(B) if out is None else out
