"""MultiScaleRoIAlign on the HIP device -- the stage in front of the interaction head.

Drop-in for `torchvision.ops.MultiScaleRoIAlign` as the reference builds it
(models/adamixer_transH_spatial_r50_models.py:158-162: featmap_names ['0','1','2','3'], output_size 7,
sampling_ratio 2) and calls it (heads/adamixer_transH_spatial_r50_head.py:387):
    box_features = box_roi_pool(features: Dict[str, Tensor[B,C,H,W]], boxes: List[Tensor[N,4]], image_shapes)
torchvision is absent from the image; its published algorithm is restated (scale inference 2**round(log2(feat/img)),
LevelMapper with canonical scale 224 / level 4 / eps 1e-6, roi_align with aligned=False).  Differentiable with respect to
the feature maps (`skg_roi_align_bwd_f32`): the reference trains the detector's backbone and neck through this pooling
(configures/hicodet/adamixer_transH_spatial_r50_main.py:109-127 gives them lr * 0.1).

Half-precision maps (all levels bf16, or all fp16) are read in place by `skg_roi_align_x`, with the arithmetic of the
fp32 kernel on the exactly widened values; `output_dtype` (default float32) picks the dtype of the pooled features, a half
output being the fp32 result rounded once.  Any other mix of map dtypes is widened to fp32 first, as before.

Channels-last maps (what a backbone run with memory_format=torch.channels_last hands over) are read in place too
(`skg_roi_align_nhwc_x`, `channels_last_route` below says when), with bit-identical results; their gradients come back
channels-last (`skg_roi_align_bwd_nhwc_f32`).  Every other layout is made [B, C, H, W]-contiguous first, as before.

`deterministic` (None: follow `torch.use_deterministic_algorithms`) selects the backward without atomics
(`skg_roi_align_bwd_det_x` / `skg_roi_align_bwd_det_nhwc_x`): a fixed summation order, the same bits on every run and in both
layouts, gradients written once in the maps' dtype into uninitialised maps (no zero fill, no fp32 temporaries).

`forward(..., mirror=[bool per image])` pools the flagged images as if their maps were mirrored along W, without the
`.flip(-1)` copy (`skg_roi_align_mirror_x` and its siblings): the kernels read column W_l - 1 - x wherever they read column x,
nothing else changes, so the output -- and the map gradients, with either backward -- have the bits of the same module on
the flipped copy.  The boxes are the caller's, in the frame of the mirrored maps (the contract of `trainer.hflip_sample`).
"""
import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn, Tensor

from . import _capi
from .engine import _stream


_HALF_CODES = {torch.float16: _capi.DTYPE_F16, torch.bfloat16: _capi.DTYPE_BF16}
_NHWC_MAX_POOLED = 8                                    # skg_roi_align_nhwc_x: larger outputs take the [B, C, H, W] route
_OUT_CODES = {torch.float32: _capi.DTYPE_F32, torch.float16: _capi.DTYPE_F16, torch.bfloat16: _capi.DTYPE_BF16}


def _level_args(feats, scales):
    L = len(feats)
    return ((C.c_void_p * L)(*[f.data_ptr() for f in feats]),
            (C.c_int32 * L)(*[int(f.shape[2]) for f in feats]), (C.c_int32 * L)(*[int(f.shape[3]) for f in feats]),
            (C.c_float * L)(*scales))


def channels_last_route(feats) -> bool:
    """True when the maps are read in place as [B, H, W, C] memory: every level channels-last and NOT also plain
    contiguous (C = 1 or H = W = 1 satisfy both: they stay on the [B, C, H, W] route), one dtype of fp32 / bf16 / fp16 for
    all levels, C % 8 == 0 and every base address 16-byte aligned (the limits of skg_roi_align_nhwc_x).  Needs no device."""
    if not feats or any(f.dim() != 4 for f in feats):
        return False
    if len({f.dtype for f in feats}) != 1 or feats[0].dtype not in _OUT_CODES:
        return False
    if feats[0].shape[1] % 8 != 0:
        return False
    return all(f.is_contiguous(memory_format=torch.channels_last) and not f.is_contiguous() and f.data_ptr() % 16 == 0
               for f in feats)


def resolve_deterministic(flag: Optional[bool]) -> bool:
    """The `deterministic` keyword of MultiScaleRoIAlign at the time of a forward call: None follows
    torch.are_deterministic_algorithms_enabled(), True / False override it."""
    if flag is None:
        return bool(torch.are_deterministic_algorithms_enabled())
    return bool(flag)


class _RoIAlignFn(torch.autograd.Function):
    """out = MultiScaleRoIAlign(feats...); backward scatters d out into zeroed feature gradients (float atomics), or, when
    cfg carries deterministic = True, gathers them in a fixed order into uninitialised maps of the maps' dtype."""

    @staticmethod
    def forward(ctx, cfg, rois, img, *feats):
        scales, k_min, k_max, canon_s, canon_l, pooled, sampling, out_dtype = cfg[:8]
        mir = cfg[9] if len(cfg) > 9 else None      # int32 flag per image on the device, or None: the entries without flags
        dts = {f.dtype for f in feats}
        nhwc = pooled <= _NHWC_MAX_POOLED and channels_last_route(feats)
        map_code = _HALF_CODES.get(feats[0].dtype) if len(dts) == 1 else None
        if nhwc:                                    # channels-last: the tensors' own storage, no copy of any level
            map_code = _OUT_CODES[feats[0].dtype]
            fs = list(feats)
        elif map_code is None:                        # fp32, fp64, mixed: widened to fp32 first
            map_code = _capi.DTYPE_F32
            fs = [f.float().contiguous() for f in feats]
        else:                                       # one half dtype: read in place (no fp32 copy of any level)
            fs = [f.contiguous() for f in feats]
        n_rois, Cc = rois.shape[0], fs[0].shape[1]
        out = torch.empty(n_rois, Cc, pooled, pooled, device=rois.device, dtype=out_dtype)
        ptrs, Hs, Ws, sc = _level_args(fs, scales)
        if mir is None:
            name, mirror_args = "skg_roi_align_nhwc_x" if nhwc else "skg_roi_align_x", ()
        else:
            name = "skg_roi_align_mirror_nhwc_x" if nhwc else "skg_roi_align_mirror_x"
            mirror_args = (mir.data_ptr(), int(mir.shape[0]))
        _capi.check(getattr(_capi.lib(), name)(ptrs, map_code, Hs, Ws, sc, len(fs), Cc, k_min, k_max, float(canon_s),
                                               int(canon_l), rois.data_ptr(), img.data_ptr(), n_rois, pooled, sampling,
                                               out.data_ptr(), _OUT_CODES[out_dtype], *mirror_args, _stream()), name)
        ctx.cfg, ctx.rois, ctx.img, ctx.mir = cfg, rois, img, mir
        ctx.shapes = [tuple(f.shape) for f in fs]
        ctx.dtypes = [f.dtype for f in feats]
        ctx.nhwc = nhwc
        ctx.det = bool(cfg[8]) if len(cfg) > 8 else False
        return out

    @staticmethod
    def backward(ctx, dout):
        scales, k_min, k_max, canon_s, canon_l, pooled, sampling = ctx.cfg[:7]
        dout = dout.float().contiguous()
        mir = ctx.mir
        fmt = torch.channels_last if ctx.nhwc else torch.contiguous_format    # gradients of channels-last maps stay so
        one = len(set(ctx.dtypes)) == 1 and ctx.dtypes[0] in _OUT_CODES
        if ctx.det:                                 # every element written once, in a fixed order: uninitialised maps
            gdt = ctx.dtypes[0] if one else torch.float32           # mixed / fp64 maps: fp32 gradients, converted below
            name = "skg_roi_align_bwd_det_nhwc_x" if ctx.nhwc else "skg_roi_align_bwd_det_x"
            dtype_arg, images_arg = (_OUT_CODES[gdt],), (ctx.shapes[0][0],)    # the two arguments only these entries take
            mirror_args = () if mir is None else (mir.data_ptr(),)
        else:                                       # float atomics into zeroed fp32 maps
            gdt = torch.float32
            name = "skg_roi_align_bwd_nhwc_f32" if ctx.nhwc else "skg_roi_align_bwd_f32"
            dtype_arg, images_arg = (), ()
            mirror_args = () if mir is None else (mir.data_ptr(), int(mir.shape[0]))
        if mir is not None:
            name = name.replace("_bwd_det_", "_bwd_det_mirror_") if ctx.det else name.replace("_bwd_", "_bwd_mirror_")
        if ctx.det:
            dfs = [torch.empty(sh, device=dout.device, dtype=gdt, memory_format=fmt) for sh in ctx.shapes]
        elif ctx.nhwc:
            dfs = [torch.empty(sh, device=dout.device, dtype=gdt, memory_format=fmt).zero_() for sh in ctx.shapes]
        else:
            dfs = [torch.zeros(sh, device=dout.device, dtype=gdt) for sh in ctx.shapes]
        ptrs, Hs, Ws, sc = _level_args(dfs, scales)
        _capi.check(getattr(_capi.lib(), name)(ptrs, *dtype_arg, Hs, Ws, sc, len(dfs), ctx.shapes[0][1], k_min, k_max,
                                               float(canon_s), int(canon_l), ctx.rois.data_ptr(), ctx.img.data_ptr(),
                                               ctx.rois.shape[0], *images_arg, pooled, sampling, dout.data_ptr(),
                                               *mirror_args, _stream()), name)
        if ctx.det and one:
            return (None, None, None) + tuple(dfs)
        return (None, None, None) + tuple(d.to(t) for d, t in zip(dfs, ctx.dtypes))


class MultiScaleRoIAlign(nn.Module):
    def __init__(self, featmap_names: List[str], output_size, sampling_ratio: int, *, canonical_scale: int = 224,
                 canonical_level: int = 4, output_dtype: Optional[torch.dtype] = None,
                 deterministic: Optional[bool] = None):
        """output_dtype: dtype of the pooled features -- None (float32, the default), torch.float32, torch.bfloat16 or
        torch.float16.
        deterministic: the backward -- None (the default) follows torch.are_deterministic_algorithms_enabled() at the
        time of the forward call, True always takes the order-fixed backward without atomics, False always the atomics."""
        super().__init__()
        if deterministic is not None and not isinstance(deterministic, bool):
            raise ValueError("deterministic must be None, True or False (got %r)" % (deterministic,))
        self.deterministic = deterministic
        if output_dtype is not None and output_dtype not in _OUT_CODES:
            raise ValueError("output_dtype must be None, torch.float32, torch.bfloat16 or torch.float16 (got %r)"
                             % (output_dtype,))
        self.output_dtype = output_dtype
        if isinstance(output_size, (tuple, list)):
            if output_size[0] != output_size[1]:
                raise ValueError("only square outputs are supported (the reference uses 7x7)")
            output_size = output_size[0]
        self.featmap_names = list(featmap_names)
        self.output_size = int(output_size)
        self.sampling_ratio = int(sampling_ratio)
        self.canonical_scale = canonical_scale
        self.canonical_level = canonical_level
        self.scales = None
        self.k_min = self.k_max = None

    def _out_dtype(self):
        dt = getattr(self, "output_dtype", None)            # (modules pickled before the keyword existed: float32)
        return torch.float32 if dt is None else dt

    def _deterministic(self) -> bool:
        return resolve_deterministic(getattr(self, "deterministic", None))   # (pickled before the keyword: None)

    @staticmethod
    def infer_scale(feature_hw, original_hw) -> float:
        """torchvision.ops.poolers._infer_scale: 2 ** round(log2(feature / image)) from the first (height) axis."""
        approx = float(feature_hw[0]) / float(original_hw[0])
        return 2.0 ** float(torch.tensor(approx).log2().round())

    def setup_scales(self, feats: List[Tensor], image_shapes: List[Tuple[int, int]]):
        max_h = max(s[0] for s in image_shapes); max_w = max(s[1] for s in image_shapes)
        self.scales = [self.infer_scale(f.shape[-2:], (max_h, max_w)) for f in feats]
        self.k_min = int(-math.log2(self.scales[0])); self.k_max = int(-math.log2(self.scales[-1]))

    def forward(self, x: Dict[str, Tensor], boxes: List[Tensor], image_shapes: List[Tuple[int, int]],
                mirror: Optional[Sequence[bool]] = None) -> Tensor:
        """mirror: None, or one bool per image -- True pools that image as if every one of its maps were mirrored along W
        (x[k][i].flip(-1)), with the same bits and without the copy; its boxes are given in the mirrored frame.  None and
        all-False are the call without the keyword: no flag array, the same launches."""
        feats = [x[k] for k in self.featmap_names if k in x]
        if not feats:
            raise KeyError("none of featmap_names %s in the feature dict" % self.featmap_names)
        if mirror is not None:
            mirror = list(mirror)
            if len(mirror) != len(boxes) or len(mirror) != int(feats[0].shape[0]):
                raise ValueError("mirror has %d flags for %d images (%d lists of boxes)"
                                 % (len(mirror), int(feats[0].shape[0]), len(boxes)))
            if not all(isinstance(m, bool) for m in mirror):
                raise ValueError("mirror must hold one bool per image (got %r)" % (mirror,))
            if not any(mirror):
                mirror = None
        dev = feats[0].device
        if dev.type != "cuda":
            raise _capi.SkgError("MultiScaleRoIAlign runs on a HIP device only")
        if self.scales is None or len(self.scales) != len(feats):
            self.setup_scales(feats, image_shapes)
        n_per = [int(b.shape[0]) for b in boxes]
        n_rois = sum(n_per)
        Cc = feats[0].shape[1]
        if n_rois == 0:
            return torch.empty(0, Cc, self.output_size, self.output_size, device=dev, dtype=self._out_dtype())
        rois = torch.cat([b.reshape(-1, 4) for b in boxes]).detach().float().contiguous()
        img = torch.repeat_interleave(torch.arange(len(boxes), dtype=torch.int32),
                                      torch.tensor(n_per)).to(dev, non_blocking=True)
        L = len(feats)
        k_min, k_max = (self.k_min, self.k_max) if L > 1 else (0, 0)
        cfg = (list(self.scales), k_min, k_max, self.canonical_scale, self.canonical_level, self.output_size,
               self.sampling_ratio, self._out_dtype(), self._deterministic(),
               None if mirror is None else torch.tensor(mirror, dtype=torch.int32).to(dev, non_blocking=True))
        if torch.is_grad_enabled() and any(f.requires_grad for f in feats):
            return _RoIAlignFn.apply(cfg, rois, img, *feats)
        return _RoIAlignFn.forward(_NoCtx(), cfg, rois, img, *feats)


class _NoCtx:
    """Stand-in for the autograd context on the no-gradient path (the forward stores a few attributes on it)."""
