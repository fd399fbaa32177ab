"""Fused optimizer step of the training loop (include/gvf_optim.h, csrc/optim.hip): everything the reference does after backward()
-- GradScaler unscale + inf check, clip_grad_norm_ over all parameters, AdamW.step per group, update_ema per rate (train_vae.py:355-375,
train_latent.py:209-225) -- as three launches and one fill over a fixed set of fp32 parameters.

`FlatGrads` is plain torch (CPU and GPU): one flat gradient buffer whose slices are the parameters' `.grad`.  `FusedAdamW` is a
`torch.optim.Optimizer` on the HIP kernels; there is no CPU fallback.

One semantic difference from stock torch.optim.AdamW: every parameter always HAS a gradient (a view of the flat buffer: zeros if nothing
flowed into it), so weight decay and the decay of the moments apply to it on every step, where stock AdamW skips a parameter whose
`.grad` is None.  DDP's gradient-bucket views behave the same way."""
import ctypes
import math
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from . import _util

_vp, _i, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t

MAX_GROUPS, MAX_EMA = 8, 4      # GVF_OPTIM_MAX_GROUPS, GVF_OPTIM_MAX_EMA
RECORD_BYTES = 128              # sizeof(gvf_optim_record)


class GvfOptimHyper(ctypes.Structure):
    _fields_ = [("n_groups", ctypes.c_int32), ("n_ema", ctypes.c_int32), ("lr", ctypes.c_double * MAX_GROUPS),
                ("weight_decay", ctypes.c_double * MAX_GROUPS), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("ema_rate", ctypes.c_double * MAX_EMA), ("max_grad_norm", ctypes.c_double)]


_lib.register({
    "gvf_optim_chunk_len": (_i, []),
    "gvf_optim_scratch_bytes": (_i, [_i64, ctypes.POINTER(_sz)]),
    "gvf_optim_norm": (_i, [_vp, _i, _vp, _i64, ctypes.POINTER(GvfOptimHyper), _vp, _vp, _vp, _sz, _vp]),
    "gvf_optim_adamw_update": (_i, [_vp, _i, _vp, _i64, ctypes.POINTER(GvfOptimHyper), _vp, _vp, _vp]),
})

# gvf_optim_tensor (72 bytes) and gvf_optim_chunk (16 bytes)
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("ema", "<u8", (MAX_EMA,)), ("group", "<i4"),
                         ("reserved", "<i4")])
CHUNK_DTYPE = np.dtype([("tensor", "<i4"), ("count", "<i4"), ("first", "<i8")])
assert TENSOR_DTYPE.itemsize == 72 and CHUNK_DTYPE.itemsize == 16


def chunk_len() -> int:
    """Elements per chunk of the library's chunk table (a multiple of 4)."""
    return int(_lib.lib().gvf_optim_chunk_len())


def build_chunk_table(sizes: Sequence[int], length: Optional[int] = None) -> np.ndarray:
    """The chunk table of tensors with `sizes` elements: a CHUNK_DTYPE array of {tensor, count, first} that covers every element of
    every tensor exactly once, in order; no chunk crosses a tensor, every chunk starts a multiple of 4 elements (of `length`) from its
    tensor's base, and a zero-element tensor has no chunk."""
    length = chunk_len() if length is None else int(length)
    if length <= 0 or length % 4:
        raise ValueError(f"build_chunk_table: chunk length {length} is not a positive multiple of 4")
    sizes = np.asarray(list(sizes), dtype=np.int64)
    if sizes.ndim != 1 or (sizes < 0).any():
        raise ValueError("build_chunk_table: sizes must be non-negative integers")
    per = (sizes + length - 1) // length
    n = int(per.sum())
    table = np.zeros(n, dtype=CHUNK_DTYPE)
    if n:
        tensor = np.repeat(np.arange(len(sizes), dtype=np.int64), per)
        start = np.cumsum(per) - per                            # index of each tensor's first chunk
        k = np.arange(n, dtype=np.int64) - start[tensor]        # chunk number within its tensor
        table["tensor"] = tensor
        table["first"] = k * length
        table["count"] = np.minimum(length, sizes[tensor] - k * length)
    return table


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


class FlatGrads:
    """One fp32 gradient buffer per device; every `requires_grad` parameter's `.grad` is a view of it that starts at a multiple of 4
    elements.  Autograd accumulates into an existing `.grad` in place, so the views persist across backward() calls; `zero_()` is one
    fill per buffer.  A gradient a parameter already holds is copied into its view."""

    def __init__(self, params: Iterable[torch.Tensor]):
        self.params: List[torch.Tensor] = []
        seen = set()
        for p in params:
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                self.params.append(p)
        if not self.params:
            raise ValueError("FlatGrads: no parameter requires grad")
        for p in self.params:
            if p.dtype != torch.float32:
                raise ValueError(f"FlatGrads: parameters must be fp32, got {p.dtype}")
        totals: Dict[torch.device, int] = {}
        self.offsets: List[int] = []
        for p in self.params:
            self.offsets.append(totals.get(p.device, 0))
            totals[p.device] = self.offsets[-1] + _pad4(p.numel())
        self.buffers: Dict[torch.device, torch.Tensor] = {d: torch.zeros(max(n, 4), dtype=torch.float32, device=d) for d, n in totals.items()}
        self.views: List[torch.Tensor] = []
        for p, off in zip(self.params, self.offsets):
            view = self.buffers[p.device][off:off + p.numel()].view(p.shape)
            if p.grad is not None:
                view.copy_(p.grad)
            p.grad = view
            self.views.append(view)

    @property
    def buffer(self) -> torch.Tensor:
        if len(self.buffers) != 1:
            raise ValueError("FlatGrads.buffer: the parameters live on several devices; use .buffers")
        return next(iter(self.buffers.values()))

    def zero_(self) -> None:
        for b in self.buffers.values():
            b.zero_()

    def attach(self) -> None:
        """Give back its view to every parameter whose `.grad` was dropped (set to None)."""
        for p, view in zip(self.params, self.views):
            if p.grad is None:
                p.grad = view

    def owns(self, params: Iterable[torch.Tensor]) -> bool:
        """True if every `requires_grad` parameter of `params` is one of this object's and its `.grad` is still the view."""
        mine = {id(p): v for p, v in zip(self.params, self.views)}
        for p in params:
            if not p.requires_grad:
                continue
            v = mine.get(id(p))
            if v is None or p.grad is None or p.grad.shape != v.shape or p.grad.dtype != v.dtype or p.grad.device != v.device:
                return False
            if v.numel() and p.grad.data_ptr() != v.data_ptr():
                return False
        return True


class FusedAdamW(torch.optim.Optimizer):
    """AdamW with decoupled weight decay, global-norm gradient clipping, loss-scale handling and EMA copies of the parameters in one
    fused device-side step (module docstring; include/gvf_optim.h for the arithmetic).

    params: parameters or parameter groups (at most 8; lr and weight_decay per group, betas and eps shared).  Every parameter that requires
    grad must be fp32, contiguous and on one GPU; parameters with requires_grad=False are left out, zero-element ones are skipped.
    ema_rates: up to 4 rates; the EMAs start as copies of the parameters.  max_grad_norm: None = no clipping.

    step(inv_scale=None): inv_scale is a 1-element fp32 device tensor (1 / the loss scale); the gradients are read as g * inv_scale.
    When their norm is not finite the step is skipped on the device (p, m, v and the step count unchanged, `found_inf` == 1) while the
    EMAs still move.  Nothing is read back to the host: `grad_norm`, `found_inf` and `clip_coef` are 0-d device tensors."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 ema_rates: Sequence[float] = (), max_grad_norm: Optional[float] = None):
        if not (lr >= 0.0 and math.isfinite(lr)):
            raise ValueError(f"FusedAdamW: invalid lr {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdamW: betas {betas} outside [0, 1)")
        if not eps > 0.0:
            raise ValueError(f"FusedAdamW: eps {eps} must be positive")
        self.ema_rates = [float(r) for r in ema_rates]
        if len(self.ema_rates) > MAX_EMA or any(not 0.0 <= r <= 1.0 for r in self.ema_rates):
            raise ValueError(f"FusedAdamW: at most {MAX_EMA} EMA rates in [0, 1], got {self.ema_rates}")
        self.max_grad_norm = max_grad_norm
        # the keys of torch.optim.AdamW's groups ride along, so that a state_dict of this optimizer drives a stock AdamW as well
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"FusedAdamW: {len(self.param_groups)} parameter groups, at most {MAX_GROUPS}")
        self._params: List[torch.Tensor] = []
        self._group_of: List[int] = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if not p.requires_grad:
                    continue
                if p.dtype != torch.float32:
                    raise ValueError(f"FusedAdamW: parameters must be fp32, got {p.dtype}")
                if not p.is_contiguous():
                    raise ValueError(f"FusedAdamW: parameters must be contiguous, got strides {p.stride()} for {tuple(p.shape)}")
                self._params.append(p)
                self._group_of.append(gi)
        if not self._params:
            raise ValueError("FusedAdamW: no parameter requires grad")
        _lib.require_cuda(*self._params)
        self.device = self._params[0].device
        if any(p.device != self.device for p in self._params):
            raise ValueError("FusedAdamW: the parameters are on several devices")
        with torch.no_grad():
            self.flat_grads = FlatGrads(self._params)
            total = self.flat_grads.buffer.numel()
            self._m = torch.zeros(total, dtype=torch.float32, device=self.device)
            self._v = torch.zeros(total, dtype=torch.float32, device=self.device)
            self._ema = [torch.zeros(total, dtype=torch.float32, device=self.device) for _ in self.ema_rates]
            self._m_views = [self._slice(self._m, i) for i in range(len(self._params))]
            self._v_views = [self._slice(self._v, i) for i in range(len(self._params))]
            self._ema_views = [[self._slice(e, i) for i in range(len(self._params))] for e in self._ema]
            for views in self._ema_views:
                for p, e in zip(self._params, views):
                    e.copy_(p)
        chunks = build_chunk_table([p.numel() for p in self._params])
        self.n_chunks = int(len(chunks))
        if self.n_chunks == 0:
            raise ValueError("FusedAdamW: every parameter is empty")
        self._chunks = torch.from_numpy(chunks.view(np.uint8).copy()).to(self.device)
        # not _util.scratch: kept for the optimizer's lifetime and zero-filled, at the exact size
        self._scratch = torch.zeros(_util.workspace_bytes("gvf_optim_scratch_bytes", self.n_chunks), dtype=torch.uint8, device=self.device)
        self._record = torch.zeros(RECORD_BYTES, dtype=torch.uint8, device=self.device)
        self._table = torch.zeros(len(self._params) * TENSOR_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self._table_ptrs = None
        self._publish_state(0)

    def _slice(self, flat: torch.Tensor, i: int) -> torch.Tensor:
        p, off = self._params[i], self.flat_grads.offsets[i]
        return flat[off:off + p.numel()].view(p.shape)

    # ------------------------------------------------------------------------------------------------------ device-side results
    @property
    def grad_norm(self) -> torch.Tensor:
        """Norm of the unscaled gradients of the last step, before clipping (0-d fp32 device tensor)."""
        return self._record[0:4].view(torch.float32)[0]

    @property
    def found_inf(self) -> torch.Tensor:
        """1 if the last step found a non-finite gradient norm and was skipped (0-d int32 device tensor)."""
        return self._record[4:8].view(torch.int32)[0]

    @property
    def clip_coef(self) -> torch.Tensor:
        return self._record[8:12].view(torch.float32)[0]

    @property
    def step_count(self) -> torch.Tensor:
        """Number of steps applied (skipped ones not counted), 0-d int64 device tensor."""
        return self._record[16:24].view(torch.int64)[0]

    def ema_params(self, k: int) -> List[torch.Tensor]:
        """The k-th EMA copy of every trainable parameter, in the order of the parameter groups (views of one flat buffer)."""
        return list(self._ema_views[k])

    def ema_state_dict(self, module: torch.nn.Module, k: int) -> dict:
        """module.state_dict() with every trainable parameter of this optimizer replaced by its k-th EMA copy (cloned)."""
        ema = {id(p): e for p, e in zip(self._params, self._ema_views[k])}
        names = {name: ema[id(p)] for name, p in module.named_parameters() if id(p) in ema}
        sd = module.state_dict()
        for name in sd:
            if name in names:
                sd[name] = names[name].detach().clone()
        return sd

    # ------------------------------------------------------------------------------------------------------------------ the step
    def _upload_table_if_changed(self) -> None:
        self.flat_grads.attach()
        for p, view in zip(self._params, self.flat_grads.views):
            if p.grad is not view and view.numel() and p.grad.data_ptr() != view.data_ptr():
                raise _lib.GvfError("FusedAdamW: a parameter's .grad was replaced; it must stay the view of the optimizer's flat buffer "
                                    "(optimizer.flat_grads)")
        ptrs = [p.data_ptr() for p in self._params]
        if ptrs == self._table_ptrs:
            return
        for p in self._params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
                raise _lib.GvfError("FusedAdamW: a parameter is no longer fp32, contiguous and on the optimizer's device")
        t = np.zeros(len(self._params), dtype=TENSOR_DTYPE)
        t["p"] = ptrs
        t["g"] = [g.data_ptr() for g in self.flat_grads.views]
        t["m"] = [m.data_ptr() for m in self._m_views]
        t["v"] = [v.data_ptr() for v in self._v_views]
        for k, views in enumerate(self._ema_views):
            t["ema"][:, k] = [e.data_ptr() for e in views]
        t["group"] = self._group_of
        self._table.copy_(torch.from_numpy(t.view(np.uint8)), non_blocking=False)
        self._table_ptrs = ptrs

    def _hyper(self) -> GvfOptimHyper:
        h = GvfOptimHyper()
        g0 = self.param_groups[0]
        h.n_groups, h.n_ema = len(self.param_groups), len(self.ema_rates)
        for gi, group in enumerate(self.param_groups):
            if tuple(group["betas"]) != tuple(g0["betas"]) or group["eps"] != g0["eps"]:
                raise ValueError("FusedAdamW: betas and eps are shared by all parameter groups")
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdamW: amsgrad and maximize are not supported")
            h.lr[gi] = float(group["lr"])
            h.weight_decay[gi] = float(group["weight_decay"])
        h.beta1, h.beta2, h.eps = float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"])
        for k, r in enumerate(self.ema_rates):
            h.ema_rate[k] = r
        h.max_grad_norm = -1.0 if self.max_grad_norm is None else float(self.max_grad_norm)
        if self.max_grad_norm is not None and not self.max_grad_norm >= 0.0:
            raise ValueError(f"FusedAdamW: max_grad_norm {self.max_grad_norm} must be None or >= 0")
        return h

    @torch.no_grad()
    def step(self, inv_scale: Optional[torch.Tensor] = None):
        """One fused step on the current stream from the gradients in the flat buffer; lr and weight decay are read from `param_groups`
        (so LambdaLR and friends work).  No host read."""
        if inv_scale is not None:
            if not isinstance(inv_scale, torch.Tensor) or inv_scale.numel() != 1 or inv_scale.dtype != torch.float32:
                raise ValueError("FusedAdamW.step: inv_scale must be a 1-element fp32 tensor")
            _lib.require_cuda(inv_scale)
            if inv_scale.device != self.device:
                raise ValueError("FusedAdamW.step: inv_scale is on another device")
        self._upload_table_if_changed()
        h = self._hyper()
        l = _lib.lib()
        stream = _lib.current_stream(self.device)
        n = len(self._params)
        with torch.cuda.device(self.device):
            _lib.check(l.gvf_optim_norm(_lib.ptr(self._table), n, _lib.ptr(self._chunks), self.n_chunks, ctypes.byref(h), _lib.ptr(inv_scale),
                                        _lib.ptr(self._record), _lib.ptr(self._scratch), self._scratch.numel(), stream), "gvf_optim_norm")
            _lib.check(l.gvf_optim_adamw_update(_lib.ptr(self._table), n, _lib.ptr(self._chunks), self.n_chunks, ctypes.byref(h),
                                                _lib.ptr(inv_scale), _lib.ptr(self._record), stream), "gvf_optim_adamw_update")
        return None

    def zero_grad(self, set_to_none: bool = True) -> None:
        """One fill of the flat gradient buffer; the views are never dropped (set_to_none is accepted and ignored)."""
        self.flat_grads.attach()
        self.flat_grads.zero_()

    # -------------------------------------------------------------------------------------------------------------- checkpoints
    def _publish_state(self, step: int) -> None:
        """self.state in torch.optim.AdamW's layout: exp_avg / exp_avg_sq are the views of the flat moment buffers."""
        self.state.clear()
        for p, m, v in zip(self._params, self._m_views, self._v_views):
            self.state[p] = {"step": torch.tensor(float(step)), "exp_avg": m, "exp_avg_sq": v}

    def state_dict(self) -> dict:
        """torch.optim.AdamW's layout (per parameter `step`, `exp_avg`, `exp_avg_sq`; loads into a stock AdamW) plus one key "ema":
        {"rates": [...], "params": [[tensor per trainable parameter] per rate]}.  Reads the step count from the device (synchronises)."""
        step = int(self.step_count.item())
        for st in self.state.values():
            st["step"] = torch.tensor(float(step))
        sd = super().state_dict()
        sd["ema"] = {"rates": list(self.ema_rates), "params": [[e.detach().clone() for e in views] for views in self._ema_views]}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        """Accepts this class's state_dict() and a stock torch.optim.AdamW's (e.g. the reference's opt*.pt): the moments are copied into
        the flat buffers and the (common) step count onto the device.  Without an "ema" key the EMAs are left as they are."""
        sd = {k: v for k, v in state_dict.items() if k != "ema"}
        super().load_state_dict(sd)
        steps = set()
        for p, m, v in zip(self._params, self._m_views, self._v_views):
            st = self.state.get(p)
            if not st:                       # stock AdamW creates no state for a parameter that never had a gradient
                m.zero_()
                v.zero_()
                continue
            if "max_exp_avg_sq" in st:
                raise ValueError("FusedAdamW.load_state_dict: amsgrad state is not supported")
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"FusedAdamW.load_state_dict: the parameters are at different steps {sorted(steps)}; the fused step keeps one count")
        step = steps.pop() if steps else 0
        self._hyper()                        # refuses groups this optimizer cannot run (amsgrad, maximize, per-group betas)
        self._record.zero_()
        self._record[16:24].view(torch.int64).fill_(step)
        self._publish_state(step)
        ema = state_dict.get("ema")
        if ema is not None:
            if [float(r) for r in ema["rates"]] != self.ema_rates:
                raise ValueError(f"FusedAdamW.load_state_dict: EMA rates {ema['rates']} do not match {self.ema_rates}")
            for views, saved in zip(self._ema_views, ema["params"]):
                if len(saved) != len(views):
                    raise ValueError("FusedAdamW.load_state_dict: EMA parameter count mismatch")
                for e, s in zip(views, saved):
                    e.copy_(s)
