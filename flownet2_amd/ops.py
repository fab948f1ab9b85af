"""Raw operator calls: torch CUDA tensors in, C ABI (libflownet2_hip.so) underneath.

torch is plumbing here (device memory + the current HIP stream); all arithmetic happens in the HIP
kernels.  Every function validates what the reference's Reshape would CHECK, then forwards to the
C entry point; there is no PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import CorrParams, L1LossParams, check


def _consts(*names):
    """The values of the headers' FN2_<name> enumerators / #defines (_lib.CONSTANTS), in the order asked for."""
    return tuple(_lib.CONSTANTS["FN2_" + n] for n in names)


MULTIPLY, SUBTRACT = _consts("CORR_MULTIPLY", "CORR_SUBTRACT")
FILL_ZERO, FILL_NAN = _consts("FILL_ZERO", "FILL_NAN")
NEAREST, LINEAR, CUBIC, AREA = _consts("RESAMPLE_NEAREST", "RESAMPLE_LINEAR", "RESAMPLE_CUBIC", "RESAMPLE_AREA")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: torch.Tensor, name: str, ndim: int = 4):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA (HIP) tensor; flownet2_amd has no CPU path")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32 (Dtype=float), got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} axes (NCHW), got shape {tuple(t.shape)}")
    return t.contiguous()


def _chk_opt(t, name: str, ndim: int = 4):
    """_chk of a blob that may be absent (a bias, a second bottom)."""
    return _chk(t, name, ndim) if t is not None else None


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _top(what: str, out, N, Cc, Ho, Wo, device):
    """The top blob of a layer: a new [N, Cc, Ho, Wo] one, or `out` (the layer writes a channel slice of it) checked against [N, *, Ho, Wo]."""
    if out is None:
        return torch.empty((N, Cc, Ho, Wo), device=device, dtype=torch.float32)
    _chk(out, "top[0]")
    if out.shape[0] != N or tuple(out.shape[2:]) != (Ho, Wo):
        raise ValueError(f"{what}: top blob {tuple(out.shape)} does not match [{N},*,{Ho},{Wo}]")
    return out


def _packed(w, n, pack, *dims):
    """n floats on w's device, filled by pack(weight, packed, *dims, stream): the operand a kernel reads."""
    packed = torch.empty(n, device=w.device, dtype=torch.float32)
    check(pack(_ptr(w), _ptr(packed), *dims, _stream()))
    return packed


def corr_params(pad=0, kernel_size=1, max_displacement=0, stride_1=1, stride_2=1, correlation_type=MULTIPLY, do_abs=False,
                single_direction=0):
    return CorrParams(int(pad), int(kernel_size), int(max_displacement), int(stride_1), int(stride_2),
                      int(correlation_type), int(bool(do_abs)), int(single_direction))


def correlation_out_shape(p: CorrParams, Cc: int, H: int, W: int):
    tc, th, tw = C.c_int(), C.c_int(), C.c_int()
    check(_lib.lib().fn2_correlation_out_shape(C.byref(p), Cc, H, W, C.byref(tc), C.byref(th), C.byref(tw)))
    return tc.value, th.value, tw.value


CORR_ROUTE_NONE, CORR_ROUTE_OWN = _consts("CORR_ROUTE_NONE", "CORR_ROUTE_OWN")    # the layer's own dispatch; CONV_ARITH_BF16X3 (below) is the arithmetic bit beside it


def correlation_forward_route(p: CorrParams, N: int, Cc: int, H: int, W: int, bf16x3: bool = False) -> int:
    """fn2_correlation_route: CORR_ROUTE_NONE for parameters correlation_out_shape refuses, CORR_ROUTE_OWN | CONV_ARITH_BF16X3 where bf16x3
    is asked for and the split-bf16 kernel (csrc/correlation_bf16x3.hip) takes the layer, CORR_ROUTE_OWN otherwise."""
    return int(_lib.lib().fn2_correlation_route(C.byref(p), int(N), int(Cc), int(H), int(W), ROUTE_BF16X3 if bf16x3 else 0))


def correlation_forward(p: CorrParams, bottom0: torch.Tensor, bottom1: torch.Tensor, out: torch.Tensor | None = None,
                        out_c0: int = 0, relu: bool = False, negative_slope: float = 0.0, bf16x3: bool = False):
    """top = Correlation(bottom0, bottom1).  With `out` wider than topC channels the layer writes the slice
    [out_c0, out_c0 + topC) of it (the Concat that follows it in FlowNetC); relu applies ReLU{negative_slope} on the way out.
    bf16x3: split-bf16 arithmetic where fn2_correlation_route hands the layer to that kernel; every other layer stays exact."""
    b0, b1 = _chk(bottom0, "bottom[0]"), _chk(bottom1, "bottom[1]")
    if b0.shape != b1.shape:   # correlation_layer.cpp:45-47
        raise ValueError("Both bottom blobs must have same shape")
    N, Cc, H, W = b0.shape
    tc, th, tw = correlation_out_shape(p, Cc, H, W)
    top = out if out is not None else torch.empty((N, tc, th, tw), device=b0.device, dtype=torch.float32)
    assert top.is_contiguous() and top.shape[0] == N and tuple(top.shape[2:]) == (th, tw) and out_c0 + tc <= top.shape[1]
    route = correlation_forward_route(p, N, Cc, H, W, bf16x3=True) if bf16x3 else CORR_ROUTE_OWN      # (exact: the one route of every layer)
    check(_lib.lib().fn2_correlation_forward_routed(C.byref(p), route, _ptr(b0), _ptr(b1), _ptr(top), N, Cc, H, W, int(top.shape[1]), int(out_c0),
                                                    int(bool(relu)), C.c_float(float(negative_slope)), None, 0, _stream()))
    return top


def correlation_backward(p: CorrParams, bottom0, bottom1, top_diff, need0=True, need1=True):
    b0, b1, td = _chk(bottom0, "bottom[0]"), _chk(bottom1, "bottom[1]"), _chk(top_diff, "top.diff")
    N, Cc, H, W = b0.shape
    d0 = torch.empty_like(b0) if need0 else None
    d1 = torch.empty_like(b1) if need1 else None
    check(_lib.lib().fn2_correlation_backward(C.byref(p), _ptr(b0), _ptr(b1), _ptr(td), _ptr(d0), _ptr(d1),
                                              N, Cc, H, W, None, 0, _stream()))
    return d0, d1


def correlation1d_out_shape(p: CorrParams, Cc: int, H: int, W: int):
    tc, th, tw = C.c_int(), C.c_int(), C.c_int()
    check(_lib.lib().fn2_correlation1d_out_shape(C.byref(p), Cc, H, W, C.byref(tc), C.byref(th), C.byref(tw)))
    return tc.value, th.value, tw.value


def correlation1d_forward(p: CorrParams, bottom0: torch.Tensor, bottom1: torch.Tensor):
    b0, b1 = _chk(bottom0, "bottom[0]"), _chk(bottom1, "bottom[1]")
    if b0.shape != b1.shape:   # correlation_layer1d.cpp:48-50
        raise ValueError("Both bottom blobs must have same shape")
    N, Cc, H, W = b0.shape
    tc, th, tw = correlation1d_out_shape(p, Cc, H, W)
    top = torch.empty((N, tc, th, tw), device=b0.device, dtype=torch.float32)
    check(_lib.lib().fn2_correlation1d_forward(C.byref(p), _ptr(b0), _ptr(b1), _ptr(top), N, Cc, H, W, _stream()))
    return top


def correlation1d_backward(p: CorrParams, bottom0, bottom1, top_diff, need0=True, need1=True):
    b0, b1, td = _chk(bottom0, "bottom[0]"), _chk(bottom1, "bottom[1]"), _chk(top_diff, "top.diff")
    N, Cc, H, W = b0.shape
    d0 = torch.empty_like(b0) if need0 else None
    d1 = torch.empty_like(b1) if need1 else None
    check(_lib.lib().fn2_correlation1d_backward(C.byref(p), _ptr(b0), _ptr(b1), _ptr(td), _ptr(d0), _ptr(d1), N, Cc, H, W, _stream()))
    return d0, d1


# codes of fn2_debug_set_correlation_impl (csrc/correlation.hip); every other value is FN2_ERR_INVALID_ARG
CORR_IMPL_AUTO = 0                # automatic choice
CORR_IMPL_GENERIC = 1             # generic (thread per element) kernels, Correlation and Correlation1D
CORR_IMPL_FWD_DWORD = 3           # general dword LDS-DMA MFMA forward even where the paired-parity kernel applies
CORR_IMPL_BWD_GEN1 = 5            # register-staged MFMA backward (corr_bwd_mfma) even where the G-ring kernel applies
CORR_IMPL_FWD_PAIR_NO_PLAN = 13   # paired-parity forward (corr_fwd_pair) without the SIMD plan
CORR_IMPL_BWD_PER_BOTTOM = 16     # one backward launch per bottom where the merged launch applies
CORR_IMPL_1D_TILED = 17           # Correlation1D: the LDS-tiled VALU forward instead of the MFMA one
CORR_IMPL_FWD_PAIR = 19           # paired-parity forward where the unit kernel applies
CORR_IMPL_UNITS = 20              # + task policy (0 .. 31): the unit kernel with that policy
CORR_IMPL_UNITS_LDS_16K = 60      # unit kernel with 16 KB of extra LDS (two workgroups per CU)
CORR_IMPL_UNITS_LDS_64K = 61      # unit kernel with 64 KB of extra LDS (one workgroup per CU)
CORR_IMPL_ABL_GLDS = 64           # + bits (0 .. 35): ablation of the general MFMA forward, FN2_ABLATION builds only
CORR_IMPL_ABL_UNITS = 100         # + bits (0 .. 63): ablation of the unit kernel, FN2_ABLATION builds only


def set_correlation_impl(impl):
    """Test / profiling hook: which correlation kernels run.  `impl` is one of the CORR_IMPL_* codes above (False / True are
    CORR_IMPL_AUTO / CORR_IMPL_GENERIC):
      CORR_IMPL_AUTO (0)              automatic choice
      CORR_IMPL_GENERIC (1)           generic kernels
      CORR_IMPL_FWD_DWORD (3)         general dword LDS-DMA forward
      CORR_IMPL_BWD_GEN1 (5)          register-staged backward
      CORR_IMPL_FWD_PAIR_NO_PLAN (13) paired-parity forward without the SIMD plan
      CORR_IMPL_BWD_PER_BOTTOM (16)   one backward launch per bottom
      CORR_IMPL_1D_TILED (17)         Correlation1D tiled VALU forward
      CORR_IMPL_FWD_PAIR (19)         paired-parity forward where the unit kernel applies
      CORR_IMPL_UNITS + policy (20 .. 51)   unit kernel with a task policy
      CORR_IMPL_UNITS_LDS_16K / _64K (60, 61)   unit kernel with extra LDS
      CORR_IMPL_ABL_GLDS + bits (64 .. 99), CORR_IMPL_ABL_UNITS + bits (100 .. 163)   ablations, FN2_ABLATION builds only
    Any other value raises Fn2Error (FN2_ERR_INVALID_ARG) and changes nothing."""
    check(_lib.lib().fn2_debug_set_correlation_impl(int(impl)))


def set_resample_generic(on):
    """Test hook: True = always the per-output-pixel Resample kernels (no integer-factor up-sampling path)."""
    check(_lib.lib().fn2_debug_set_resample_generic(int(bool(on))))


def flow_warp_forward(image, flow, fill_value=FILL_ZERO):
    im, fl = _chk(image, "bottom[0] (image)"), _chk(flow, "bottom[1] (flow)")
    N, Cc, H, W = im.shape
    if fl.shape[0] != N:
        raise ValueError("Num of the inputs should be the same")               # flow_warp_layer.cpp:45
    if fl.shape[1] != 2:
        raise ValueError("Flow should have 2 channels: x-flow and y-flow")     # :46
    if fl.shape[3] != W or fl.shape[2] != H:
        raise ValueError("Width/Height of the inputs should be the same")      # :47-48
    out = torch.empty_like(im)
    check(_lib.lib().fn2_flow_warp_forward(_ptr(im), _ptr(fl), _ptr(out), N, Cc, H, W, int(fill_value), _stream()))
    return out


def _as_slice(arg, what):
    """A blob argument of the *_slices entry points: a plain [N,C,H,W] tensor, or (blob, c0, C) = channels [c0, c0 + C) of a wider
    contiguous blob.  -> (blob, channels of the blob, c0, C)."""
    if isinstance(arg, tuple):
        blob, c0, Cc = arg
        if isinstance(blob, torch.Tensor) and not blob.is_contiguous():
            raise ValueError(what + ": a sliced blob must be contiguous")
        blob = _chk(blob, what)
        if c0 < 0 or Cc < 1 or c0 + Cc > blob.shape[1]:
            raise ValueError("%s: channel slice [%d, %d) outside a blob of %d channels" % (what, c0, c0 + Cc, blob.shape[1]))
        return blob, int(blob.shape[1]), int(c0), int(Cc)
    t = _chk(arg, what)
    return t, int(t.shape[1]), 0, int(t.shape[1])


def flow_warp_forward_slices(image, flow, out=None, fill_value=FILL_ZERO):
    """FlowWarp whose image bottom and top may be channel slices (blob, c0, C) of wider blobs (the Concat around it disappears).
    Returns the top blob (a new [N,C,H,W] one if `out` is None)."""
    im, ictot, ic0, Cc = _as_slice(image, "bottom[0] (image)")
    fl, fctot, fc0, Cf = _as_slice(flow, "bottom[1] (flow)")
    N, _, H, W = im.shape
    if fl.shape[0] != N or Cf != 2 or tuple(fl.shape[2:]) != (H, W):
        raise ValueError("flow_warp: flow must be [N,2,H,W] of the image's size")
    if out is None:
        out = torch.empty((N, Cc, H, W), device=im.device, dtype=torch.float32)
    top, octot, oc0, Co = _as_slice(out, "top[0]")
    if Co != Cc or top.shape[0] != N or tuple(top.shape[2:]) != (H, W):
        raise ValueError("flow_warp: top slice does not match the image")
    check(_lib.lib().fn2_flow_warp_forward_slices(_ptr(im), ictot, ic0, _ptr(fl), fctot, fc0, _ptr(top), octot, oc0, N, Cc, H, W, int(fill_value), _stream()))
    return top


def flow_warp_backward(image, flow, warped_diff, propagate_image=True, propagate_flow=True):
    im, fl, wd = _chk(image, "image"), _chk(flow, "flow"), _chk(warped_diff, "top.diff")
    N, Cc, H, W = im.shape
    di, df = torch.empty_like(im), torch.empty_like(fl)
    nbytes = _lib.lib().fn2_flow_warp_backward_workspace_bytes(N, Cc, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=im.device)
    check(_lib.lib().fn2_flow_warp_backward(_ptr(im), _ptr(fl), _ptr(wd), _ptr(di), _ptr(df), N, Cc, H, W,
                                            int(propagate_image), int(propagate_flow), _ptr(ws), nbytes, _stream()))
    return di, df


def resample_forward(x, height, width, type=LINEAR, antialias=True):
    x = _chk(x, "bottom[0]")
    N, Cc, H, W = x.shape
    if height < 1 or width < 1:
        raise ValueError("ResampleLayer must have top_height > 0 and top_width > 0")
    out = torch.empty((N, Cc, int(height), int(width)), device=x.device, dtype=torch.float32)
    check(_lib.lib().fn2_resample_forward(_ptr(x), _ptr(out), N, Cc, H, W, int(height), int(width), int(type), int(bool(antialias)), _stream()))
    return out


def resample_forward_slices(x, height, width, type=LINEAR, antialias=True, in_scale=1.0, out=None, out2=None, out2_scale=1.0):
    """Resample(x * in_scale) into a channel slice `out` = (blob, c0, C) (a new blob if None); out2 (optional slice) = top * out2_scale.
    The Eltwise scalings and the Concat the FlowNet2 graphs put around the layer, without their passes.  Returns the `out` blob."""
    x = _chk(x, "bottom[0]")
    N, Cc, H, W = x.shape
    if height < 1 or width < 1:
        raise ValueError("ResampleLayer must have top_height > 0 and top_width > 0")
    if out is None:
        out = torch.empty((N, Cc, int(height), int(width)), device=x.device, dtype=torch.float32)
    top, octot, oc0, Co = _as_slice(out, "top[0]")
    if Co != Cc or top.shape[0] != N or tuple(top.shape[2:]) != (int(height), int(width)):
        raise ValueError("resample: top slice does not match")
    t2, o2ctot, o2c0 = None, 0, 0
    if out2 is not None:
        t2, o2ctot, o2c0, C2 = _as_slice(out2, "top[1]")
        if C2 != Cc or t2.shape[0] != N or tuple(t2.shape[2:]) != (int(height), int(width)):
            raise ValueError("resample: second top slice does not match")
    check(_lib.lib().fn2_resample_forward_slices(_ptr(x), C.c_float(float(in_scale)), _ptr(top), octot, oc0, _ptr(t2), o2ctot, o2c0,
                                                 C.c_float(float(out2_scale)), N, Cc, H, W, int(height), int(width), int(type),
                                                 int(bool(antialias)), _stream()))
    return top


def l1_params(l2_per_location=False, l2_prescale_by_channels=False, normalize_by_num_entries=False, epsilon=1e-2, plateau=0.0):
    return L1LossParams(int(bool(l2_per_location)), int(bool(l2_prescale_by_channels)), int(bool(normalize_by_num_entries)),
                        float(epsilon), float(plateau))


def l1loss_workspace(x: torch.Tensor) -> torch.Tensor:
    N, Cc, H, W = x.shape
    nbytes = _lib.lib().fn2_l1loss_workspace_bytes(N, Cc, H, W)
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device)


def l1loss_forward(p: L1LossParams, bottom0, bottom1=None, workspace=None):
    """Returns (loss [0-axis device tensor], workspace).  workspace[:8] viewed as float32 = {loss, normalize_coeff}."""
    b0 = _chk(bottom0, "bottom[0]")
    b1 = _chk_opt(bottom1, "bottom[1]")
    if b1 is not None and b1.shape != b0.shape:
        raise ValueError("L1Loss: bottom blobs must have the same shape")
    N, Cc, H, W = b0.shape
    ws = workspace if workspace is not None else l1loss_workspace(b0)
    loss = torch.empty((), device=b0.device, dtype=torch.float32)
    check(_lib.lib().fn2_l1loss_forward(C.byref(p), _ptr(b0), _ptr(b1), _ptr(loss), N, Cc, H, W, _ptr(ws), ws.numel(), _stream()))
    return loss, ws


def l1loss_backward(p: L1LossParams, bottom0, bottom1, top_diff: float, workspace):
    b0 = _chk(bottom0, "bottom[0]")
    b1 = _chk_opt(bottom1, "bottom[1]")
    N, Cc, H, W = b0.shape
    d0 = torch.empty_like(b0)
    d1 = torch.empty_like(b0) if b1 is not None else None
    check(_lib.lib().fn2_l1loss_backward(C.byref(p), _ptr(b0), _ptr(b1), C.c_float(float(top_diff)), _ptr(d0), _ptr(d1),
                                         N, Cc, H, W, _ptr(workspace), workspace.numel(), _stream()))
    return d0, d1


_L1_SYNC = {}       # (device, stream) -> the zeroed arrival counters of fn2_l1loss_forward_multi (every call leaves them zero)


def _l1_scales(bottoms0, bottoms1, weights, diffs0=None, diffs1=None):
    n = len(bottoms0)
    arr = (_lib.L1LossScale * n)()
    for k in range(n):
        b0 = _chk(bottoms0[k], "bottom[0]")
        b1 = _chk(bottoms1[k], "bottom[1]") if bottoms1 is not None and bottoms1[k] is not None else None
        if b1 is not None and b1.shape != b0.shape:
            raise ValueError("L1Loss: bottom blobs must have the same shape")
        N, Cc, H, W = b0.shape
        arr[k].bottom0, arr[k].bottom1 = b0.data_ptr(), (b1.data_ptr() if b1 is not None else None)
        arr[k].bottom0_diff = diffs0[k].data_ptr() if diffs0 is not None else None
        arr[k].bottom1_diff = diffs1[k].data_ptr() if diffs1 is not None and diffs1[k] is not None else None
        arr[k].N, arr[k].C, arr[k].H, arr[k].W = N, Cc, H, W
        arr[k].loss_weight = float(weights[k])
    return arr


def l1loss_forward_multi(p: L1LossParams, bottoms0, bottoms1, weights):
    """Every L1Loss layer of a net in one launch (csrc/l1loss.hip: l1loss_fwd_multi).  Returns (total [0-axis device tensor] =
    sum_k weights[k] * loss_k in list order, losses [n], workspace); per scale bit-identical to l1loss_forward."""
    n = len(bottoms0)
    dev = bottoms0[0].device
    ws = torch.empty(int(_lib.lib().fn2_l1loss_multi_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    key = (dev.index, int(torch.cuda.current_stream().cuda_stream))
    sync = _L1_SYNC.get(key)
    if sync is None:
        sync = _L1_SYNC[key] = torch.zeros(int(_lib.lib().fn2_l1loss_multi_sync_bytes()), dtype=torch.uint8, device=dev)
    losses = torch.empty((n,), device=dev, dtype=torch.float32)
    total = torch.empty((), device=dev, dtype=torch.float32)
    arr = _l1_scales(bottoms0, bottoms1, weights)
    check(_lib.lib().fn2_l1loss_forward_multi(C.byref(p), n, arr, _ptr(losses), _ptr(total), _ptr(ws), ws.numel(), _ptr(sync), _stream()))
    return total, losses, ws


def l1loss_backward_multi(p: L1LossParams, bottoms0, bottoms1, weights, total_diff, workspace, need1=False):
    """Gradients of every scale for d(objective) / d(total) = total_diff (a DEVICE scalar tensor, or None for 1) in one launch."""
    n = len(bottoms0)
    d0 = [torch.empty_like(b) for b in bottoms0]
    d1 = [torch.empty_like(b) if (need1 and bottoms1 is not None and bottoms1[k] is not None) else None for k, b in enumerate(bottoms0)]
    arr = _l1_scales(bottoms0, bottoms1, weights, d0, d1)
    td = _chk(total_diff.reshape(1), "total_diff", ndim=1) if total_diff is not None else None
    check(_lib.lib().fn2_l1loss_backward_multi(C.byref(p), n, arr, _ptr(td), _ptr(workspace), workspace.numel(), _stream()))
    return d0, d1


def lpq_params(p, q, p_epsilon=0.0, q_epsilon=1e-2, l2_prescale_by_channels=False, normalize_by_num_entries=False):
    """The per-call arguments of the fn2_lpq_loss_* entry points, in their order (include/flownet2_hip_lpq_loss.h)."""
    return (C.c_float(float(p)), C.c_float(float(q)), C.c_float(float(p_epsilon)), C.c_float(float(q_epsilon)),
            int(bool(l2_prescale_by_channels)), int(bool(normalize_by_num_entries)))


def lpq_loss_sizes(nscales: int = 1):
    """(workspace bytes of one layer, of `nscales` layers in one launch, bytes of the arrival counters)."""
    one, multi, sync = C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(_lib.lib().fn2_lpq_loss_sizes(int(nscales), C.byref(one), C.byref(multi), C.byref(sync)))
    return one.value, multi.value, sync.value


def lpq_loss_forward(params, bottom0, bottom1=None, workspace=None):
    """LpqLoss forward (csrc/lpq_loss.hip); params = lpq_params(...).  Returns (loss [0-axis device tensor], workspace);
    workspace[:8] viewed as float32 = {loss, normalize_coeff}."""
    b0 = _chk(bottom0, "bottom[0]")
    b1 = _chk_opt(bottom1, "bottom[1]")
    if b1 is not None and b1.shape != b0.shape:
        raise ValueError("LpqLoss: bottom blobs must have the same shape")
    N, Cc, H, W = b0.shape
    ws = workspace if workspace is not None else torch.empty(lpq_loss_sizes()[0], dtype=torch.uint8, device=b0.device)
    loss = torch.empty((), device=b0.device, dtype=torch.float32)
    check(_lib.lib().fn2_lpq_loss_forward(_ptr(b0), _ptr(b1), _ptr(loss), N, Cc, H, W, *params, _ptr(ws), ws.numel(), _stream()))
    return loss, ws


def lpq_loss_backward(params, bottom0, bottom1, top_diff: float, workspace):
    b0 = _chk(bottom0, "bottom[0]")
    b1 = _chk_opt(bottom1, "bottom[1]")
    N, Cc, H, W = b0.shape
    d0 = torch.empty_like(b0)
    d1 = torch.empty_like(b0) if b1 is not None else None
    check(_lib.lib().fn2_lpq_loss_backward(_ptr(b0), _ptr(b1), C.c_float(float(top_diff)), _ptr(d0), _ptr(d1), N, Cc, H, W, *params,
                                           _ptr(workspace), workspace.numel(), _stream()))
    return d0, d1


_LPQ_SYNC = {}      # (device, stream) -> the zeroed arrival counters of fn2_lpq_loss_forward_multi (every call leaves them zero)


def _lpq_scales(bottoms0, bottoms1, weights):
    """The host arrays of a _multi call: (b0 pointers, b1 pointers, shapes [4 n], loss weights) and the checked tensors they point into."""
    n = len(bottoms0)
    b0s = [_chk(b, "bottom[0]") for b in bottoms0]
    b1s = [_chk_opt(bottoms1[k], "bottom[1]") if bottoms1 is not None else None for k in range(n)]
    for b0, b1 in zip(b0s, b1s):
        if b1 is not None and b1.shape != b0.shape:
            raise ValueError("LpqLoss: bottom blobs must have the same shape")
    shapes = (C.c_int * (4 * n))(*[int(d) for b in b0s for d in b.shape])
    return _ptr_array(b0s), _ptr_array(b1s), shapes, (C.c_float * n)(*[float(w) for w in weights]), b0s, b1s


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def lpq_loss_forward_multi(params, bottoms0, bottoms1, weights):
    """Every LpqLoss layer of a net in one launch (csrc/lpq_loss.hip: lpq_fwd_multi).  Returns (total [0-axis device tensor] =
    sum_k weights[k] * loss_k in list order, losses [n], workspace); per scale bit-identical to lpq_loss_forward."""
    n = len(bottoms0)
    dev = bottoms0[0].device
    _, ws_bytes, sync_bytes = lpq_loss_sizes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    key = (dev.index, int(torch.cuda.current_stream().cuda_stream))
    sync = _LPQ_SYNC.get(key)
    if sync is None:
        sync = _LPQ_SYNC[key] = torch.zeros(sync_bytes, dtype=torch.uint8, device=dev)
    losses = torch.empty((n,), device=dev, dtype=torch.float32)
    total = torch.empty((), device=dev, dtype=torch.float32)
    p0, p1, shapes, lw, _b0s, _b1s = _lpq_scales(bottoms0, bottoms1, weights)
    check(_lib.lib().fn2_lpq_loss_forward_multi(n, p0, p1, shapes, lw, *params, _ptr(losses), _ptr(total), _ptr(ws), ws.numel(), _ptr(sync),
                                                _stream()))
    return total, losses, ws


def lpq_loss_backward_multi(params, bottoms0, bottoms1, weights, total_diff, workspace, need1=False):
    """Gradients of every scale for d(objective) / d(total) = total_diff (a DEVICE scalar tensor, or None for 1) in one launch."""
    n = len(bottoms0)
    p0, p1, shapes, lw, b0s, b1s = _lpq_scales(bottoms0, bottoms1, weights)
    d0 = [torch.empty_like(b) for b in b0s]
    d1 = [torch.empty_like(b) if (need1 and b1s[k] is not None) else None for k, b in enumerate(b0s)]
    td = _chk(total_diff.reshape(1), "total_diff", ndim=1) if total_diff is not None else None
    check(_lib.lib().fn2_lpq_loss_backward_multi(n, p0, p1, _ptr_array(d0), _ptr_array(d1), shapes, lw, *params, _ptr(td), _ptr(workspace),
                                                 workspace.numel(), _stream()))
    return d0, d1


_FLOW_METRICS_K = _lib.FLOW_METRICS_CONSTANTS["FN2_FLOW_METRICS_K"]      # columns of a results row (evaluate.COLUMNS names them)


def flow_metrics_sizes(N: int, H: int, W: int):
    """(workspace bytes for [N,2,H,W], K) of fn2_flow_metrics (include/flownet2_hip_flow_metrics.h)."""
    nbytes, k = C.c_size_t(), C.c_int()
    check(_lib.lib().fn2_flow_metrics_sizes(int(N), int(H), int(W), C.byref(nbytes), C.byref(k)))
    return nbytes.value, k.value


def flow_metrics(pred, gt, valid=None, occ=None, outlier=(3.0, 0.05), bands=(10.0, 40.0), epe_map=False):
    """Flow error metrics (csrc/flow_metrics.hip) of pred against gt [N,2,H,W]; valid / occ [N,1,H,W] or None.  Returns (results
    [N + 1, K] float64 on the device: one row per sample and the totals row, columns evaluate.COLUMNS; the epe map [N,1,H,W] or None)."""
    p, g = _chk(pred, "pred"), _chk(gt, "gt")
    if p.shape != g.shape or p.shape[1] != 2:
        raise ValueError(f"flow_metrics: pred {tuple(p.shape)} and gt {tuple(g.shape)} must both be [N,2,H,W]")
    N, _, H, W = p.shape
    v, o = _chk_opt(valid, "valid"), _chk_opt(occ, "occ")
    for name, m in (("valid", v), ("occ", o)):
        if m is not None and tuple(m.shape) != (N, 1, H, W):
            raise ValueError(f"flow_metrics: {name} {tuple(m.shape)} must be [{N},1,{H},{W}]")
    ws = torch.empty(flow_metrics_sizes(N, H, W)[0], dtype=torch.uint8, device=p.device)
    results = torch.empty((N + 1, _FLOW_METRICS_K), dtype=torch.float64, device=p.device)
    emap = torch.empty((N, 1, H, W), dtype=torch.float32, device=p.device) if epe_map else None
    check(_lib.lib().fn2_flow_metrics(_ptr(p), _ptr(g), _ptr(v), _ptr(o), N, H, W, C.c_float(float(outlier[0])), C.c_float(float(outlier[1])),
                                      C.c_float(float(bands[0])), C.c_float(float(bands[1])), _ptr(results), _ptr(emap), _ptr(ws), ws.numel(),
                                      _stream()))
    return results, emap


_FLOW_CONSISTENCY_K = _lib.FLOW_CONSISTENCY_CONSTANTS["FN2_FLOW_CONSISTENCY_K"]      # columns of a results row (evaluate.CONSISTENCY_COLUMNS)


def flow_consistency_sizes(N: int, H: int, W: int):
    """(workspace bytes for [N,2,H,W], K) of fn2_flow_consistency (include/flownet2_hip_flow_consistency.h)."""
    nbytes, k = C.c_size_t(), C.c_int()
    check(_lib.lib().fn2_flow_consistency_sizes(int(N), int(H), int(W), C.byref(nbytes), C.byref(k)))
    return nbytes.value, k.value


def flow_consistency(fw, bw, alpha=(0.01, 0.5), beta=(0.01, 0.002), flags=False, err=False, warped=False):
    """Forward-backward consistency (csrc/flow_consistency.hip) of fw (frame 0 -> 1) and bw (frame 1 -> 0), both [N,2,H,W].  Returns
    (results [2, N + 1, K] float64 on the device: per direction one row per sample and the totals row, columns
    evaluate.CONSISTENCY_COLUMNS; occ, flags, err, warped: each a (forward, backward) pair of maps, or None where not asked for)."""
    f, b = _chk(fw, "fw"), _chk(bw, "bw")
    if f.shape != b.shape or f.shape[1] != 2:
        raise ValueError(f"flow_consistency: fw {tuple(f.shape)} and bw {tuple(b.shape)} must both be [N,2,H,W]")
    if f.device != b.device:
        raise ValueError(f"flow_consistency: fw on {f.device}, bw on {b.device}")
    N, _, H, W = f.shape
    ws = torch.empty(flow_consistency_sizes(N, H, W)[0], dtype=torch.uint8, device=f.device)
    results = torch.empty((2, N + 1, _FLOW_CONSISTENCY_K), dtype=torch.float64, device=f.device)
    pair = lambda want, ch, dtype: tuple(torch.empty((N, ch, H, W), dtype=dtype, device=f.device) for _ in range(2)) if want else None
    occ, fl, er, wa = pair(True, 1, torch.float32), pair(flags, 1, torch.uint8), pair(err, 1, torch.float32), pair(warped, 2, torch.float32)
    two = lambda p: (_ptr(p[0]), _ptr(p[1])) if p is not None else (_ptr(None), _ptr(None))
    check(_lib.lib().fn2_flow_consistency(_ptr(f), _ptr(b), N, H, W, C.c_float(float(alpha[0])), C.c_float(float(alpha[1])),
                                          C.c_float(float(beta[0])), C.c_float(float(beta[1])), _ptr(results), *two(fl), *two(occ), *two(er),
                                          *two(wa), _ptr(ws), ws.numel(), _stream()))
    return results, occ, fl, er, wa


_UNSUP_LOSS_K = _lib.UNSUP_LOSS_CONSTANTS["FN2_UNSUP_LOSS_K"]      # columns of a results row (evaluate.UNSUP_LOSS_COLUMNS)


def unsup_loss_sizes(N: int, H: int, W: int):
    """(workspace bytes for [N,*,H,W], K) of fn2_unsup_loss_forward (include/flownet2_hip_unsup_loss.h)."""
    nbytes, k = C.c_size_t(), C.c_int()
    check(_lib.lib().fn2_unsup_loss_sizes(int(N), int(H), int(W), C.byref(nbytes), C.byref(k)))
    return nbytes.value, k.value


def unsup_loss_params(data_weight=1.0, smooth_weight=1.0, charbonnier=(1e-3, 0.45), smooth_charbonnier=(1e-3, 0.45), edge_weight=10.0,
                      smooth_order=2, flow_mult=1.0):
    """The scalar arguments of fn2_unsup_loss_forward / _backward, in their order, as ctypes values."""
    (eps_d, gamma_d), (eps_s, gamma_s) = charbonnier, smooth_charbonnier
    return (*(C.c_float(float(v)) for v in (data_weight, smooth_weight, eps_d, gamma_d, eps_s, gamma_s, edge_weight)), int(smooth_order),
            C.c_float(float(flow_mult)))


def _unsup_loss_blobs(what, img0, img1, fw, bw, occ_fw, occ_bw):
    i0, i1, f = _chk(img0, "img0"), _chk(img1, "img1"), _chk(fw, "fw")
    b, of, ob = _chk_opt(bw, "bw"), _chk_opt(occ_fw, "occ_fw"), _chk_opt(occ_bw, "occ_bw")
    N, Cc, H, W = i0.shape
    if i1.shape != i0.shape:
        raise ValueError(f"{what}: img0 {tuple(i0.shape)} and img1 {tuple(i1.shape)} must have one shape")
    for name, t, ch in (("fw", f, 2), ("bw", b, 2), ("occ_fw", of, 1), ("occ_bw", ob, 1)):
        if t is not None and tuple(t.shape) != (N, ch, H, W):
            raise ValueError(f"{what}: {name} {tuple(t.shape)} must be [{N},{ch},{H},{W}]")
        if t is not None and t.device != i0.device:
            raise ValueError(f"{what}: {name} on {t.device}, img0 on {i0.device}")
    if i1.device != i0.device:
        raise ValueError(f"{what}: img1 on {i1.device}, img0 on {i0.device}")
    if ob is not None and b is None:
        raise ValueError(f"{what}: occ_bw without a bw")
    return (i0, i1, f, b, of, ob), (N, Cc, H, W)


def unsup_loss_forward(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, params=None, loss=True):
    """The unsupervised loss (csrc/unsup_loss.hip) of fw (frame 0 -> 1) and, where given, bw (frame 1 -> 0) [N,2,H,W] on the images
    [N,C,H,W]; occ_* [N,1,H,W] or None; params: unsup_loss_params(...).  Returns (results [2, N + 1, K] float64 on the device: per
    direction one row per sample and the totals row, columns evaluate.UNSUP_LOSS_COLUMNS; the loss, a 0-axis device tensor, or None)."""
    blobs, (N, Cc, H, W) = _unsup_loss_blobs("unsup_loss_forward", img0, img1, fw, bw, occ_fw, occ_bw)
    dev = blobs[0].device
    ws = torch.empty(unsup_loss_sizes(N, H, W)[0], dtype=torch.uint8, device=dev)
    results = torch.empty((2, N + 1, _UNSUP_LOSS_K), dtype=torch.float64, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev) if loss else None
    check(_lib.lib().fn2_unsup_loss_forward(*(_ptr(t) for t in blobs), N, Cc, H, W, *(params or unsup_loss_params()), _ptr(results), _ptr(out),
                                            _ptr(ws), ws.numel(), _stream()))
    return results, out


def unsup_loss_backward(img0, img1, fw, bw, occ_fw, occ_bw, params, results, total_diff=None, need_bw=True):
    """The gradient of unsup_loss_forward's loss for fw and (need_bw, with a bw) bw, times total_diff (a device scalar; None: 1);
    results: what the forward returned for the same inputs.  Returns (fw_diff, bw_diff or None), each [N,2,H,W]."""
    blobs, (N, Cc, H, W) = _unsup_loss_blobs("unsup_loss_backward", img0, img1, fw, bw, occ_fw, occ_bw)
    dev = blobs[0].device
    if not isinstance(results, torch.Tensor) or results.dtype != torch.float64 or tuple(results.shape) != (2, N + 1, _UNSUP_LOSS_K) or \
            results.device != dev or not results.is_contiguous():
        raise ValueError(f"unsup_loss_backward: results must be the forward's float64 [2,{N + 1},{_UNSUP_LOSS_K}] on {dev}")
    g = None
    if total_diff is not None:
        g = _chk(total_diff, "total_diff", None)
        if g.numel() != 1 or g.device != dev:
            raise ValueError(f"unsup_loss_backward: total_diff must be one float on {dev}")
    fd = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev)
    bd = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev) if need_bw and blobs[3] is not None else None
    check(_lib.lib().fn2_unsup_loss_backward(*(_ptr(t) for t in blobs), N, Cc, H, W, *params, _ptr(results), _ptr(g), _ptr(fd), _ptr(bd),
                                             _stream()))
    return fd, bd


_CENSUS_LOSS_K = _lib.CENSUS_LOSS_CONSTANTS["FN2_CENSUS_LOSS_K"]      # columns of a results row (evaluate.CENSUS_LOSS_COLUMNS)


def census_loss_sizes(N: int, H: int, W: int, radius: int = 3):
    """(workspace bytes, floats of `saved`, K) of fn2_census_loss_forward for [N,*,H,W] (include/flownet2_hip_census_loss.h)."""
    nbytes, nsaved, k = C.c_size_t(), C.c_size_t(), C.c_int()
    check(_lib.lib().fn2_census_loss_sizes(int(N), int(H), int(W), int(radius), C.byref(nbytes), C.byref(nsaved), C.byref(k)))
    return nbytes.value, nsaved.value, k.value


def census_loss_params(data_weight=1.0, charbonnier=(1e-3, 0.45), radius=3, census_eps=(0.81, 0.1), intensity_scale=255.0, flow_mult=1.0):
    """The scalar arguments of fn2_census_loss_forward / _backward, in their order, as ctypes values."""
    (eps_d, gamma_d), (c_t, c_h) = charbonnier, census_eps
    f = lambda v: C.c_float(float(v))
    return (f(data_weight), f(eps_d), f(gamma_d), int(radius), f(c_t), f(c_h), f(intensity_scale), f(flow_mult))


def census_loss_forward(img0, img1, fw, bw=None, occ_fw=None, occ_bw=None, params=None, loss=True, save=True):
    """The census data term (csrc/census_loss.hip) of fw (frame 0 -> 1) and, where given, bw (frame 1 -> 0) [N,2,H,W] on the images
    [N,C,H,W]; occ_* [N,1,H,W] or None; params: census_loss_params(...).  Returns (results [2, N + 1, K] float64 on the device: per
    direction one row per sample and the totals row, columns evaluate.CENSUS_LOSS_COLUMNS; the loss, a 0-axis device tensor, or None;
    saved [2,N,3,H,W], the planes G, Wg and pd the backward reads, or None)."""
    blobs, (N, Cc, H, W) = _unsup_loss_blobs("census_loss_forward", img0, img1, fw, bw, occ_fw, occ_bw)
    dev = blobs[0].device
    params = params or census_loss_params()
    ws = torch.empty(census_loss_sizes(N, H, W, params[3])[0], dtype=torch.uint8, device=dev)
    results = torch.empty((2, N + 1, _CENSUS_LOSS_K), dtype=torch.float64, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev) if loss else None
    saved = torch.empty((2, N, 3, H, W), dtype=torch.float32, device=dev) if save else None
    check(_lib.lib().fn2_census_loss_forward(*(_ptr(t) for t in blobs), N, Cc, H, W, *params, _ptr(results), _ptr(out), _ptr(saved), _ptr(ws),
                                             ws.numel(), _stream()))
    return results, out, saved


def census_loss_backward(img0, img1, fw, bw, params, results, saved, total_diff=None, need_bw=True):
    """The gradient of census_loss_forward's loss for fw and (need_bw, with a bw) bw, times total_diff (a device scalar; None: 1);
    results, saved: what the forward returned for the same inputs.  Returns (fw_diff, bw_diff or None), each [N,2,H,W]."""
    blobs, (N, Cc, H, W) = _unsup_loss_blobs("census_loss_backward", img0, img1, fw, bw, None, None)
    dev = blobs[0].device
    if not isinstance(results, torch.Tensor) or results.dtype != torch.float64 or tuple(results.shape) != (2, N + 1, _CENSUS_LOSS_K) or \
            results.device != dev or not results.is_contiguous():
        raise ValueError(f"census_loss_backward: results must be the forward's float64 [2,{N + 1},{_CENSUS_LOSS_K}] on {dev}")
    if not isinstance(saved, torch.Tensor) or saved.dtype != torch.float32 or tuple(saved.shape) != (2, N, 3, H, W) or saved.device != dev or \
            not saved.is_contiguous():
        raise ValueError(f"census_loss_backward: saved must be the forward's float32 [2,{N},3,{H},{W}] on {dev}")
    g = None
    if total_diff is not None:
        g = _chk(total_diff, "total_diff", None)
        if g.numel() != 1 or g.device != dev:
            raise ValueError(f"census_loss_backward: total_diff must be one float on {dev}")
    fd = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev)
    bd = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev) if need_bw and blobs[3] is not None else None
    check(_lib.lib().fn2_census_loss_backward(*(_ptr(t) for t in blobs[:4]), N, Cc, H, W, *params, _ptr(results), _ptr(saved), _ptr(g), _ptr(fd),
                                              _ptr(bd), _stream()))
    return fd, bd


_FLOW_SPLAT_K = _lib.FLOW_SPLAT_CONSTANTS["FN2_FLOW_SPLAT_K"]      # columns of a results row (evaluate.FLOW_SPLAT_COLUMNS)
_FLOW_SPLAT_IMPORTANCES = {n[len("FN2_FLOW_SPLAT_IMPORTANCE_"):].lower(): v for n, v in _lib.FLOW_SPLAT_CONSTANTS.items()
                           if n.startswith("FN2_FLOW_SPLAT_IMPORTANCE_")}      # none, linear, softmax


def flow_splat_sizes(N: int, C_: int, H: int, W: int):
    """(workspace bytes for [N,C,H,W], K) of fn2_flow_splat_forward (include/flownet2_hip_flow_splat.h)."""
    nbytes, k = C.c_size_t(), C.c_int()
    check(_lib.lib().fn2_flow_splat_sizes(int(N), int(C_), int(H), int(W), C.byref(nbytes), C.byref(k)))
    return nbytes.value, k.value


def _flow_splat_blobs(what, values, flow, metric, src_valid):
    v, f = _chk(values, "values"), _chk(flow, "flow")
    z, m = _chk_opt(metric, "metric"), _chk_opt(src_valid, "src_valid")
    N, Cc, H, W = v.shape
    for name, t, ch in (("flow", f, 2), ("metric", z, 1), ("src_valid", m, 1)):
        if t is not None and tuple(t.shape) != (N, ch, H, W):
            raise ValueError(f"{what}: {name} {tuple(t.shape)} must be [{N},{ch},{H},{W}]")
        if t is not None and t.device != v.device:
            raise ValueError(f"{what}: {name} on {t.device}, values on {v.device}")
    return (v, f, z, m), (N, Cc, H, W)


def _flow_splat_importance(what, importance):
    if importance not in _FLOW_SPLAT_IMPORTANCES:
        raise ValueError(f"{what}: importance must be one of {sorted(_FLOW_SPLAT_IMPORTANCES)}, got {importance!r}")
    return _FLOW_SPLAT_IMPORTANCES[importance]


def flow_splat_forward(values, flow, metric=None, src_valid=None, t=1.0, importance="none", normalize=False, fill_value=FILL_ZERO, out=True,
                       weight=True, hole=False, status=False):
    """Forward warping (csrc/flow_splat.hip): values [N,C,H,W] carried along t * flow [N,2,H,W] and spread over the four cells around the
    landing point, weighted by metric [N,1,H,W] (importance "linear": z, "softmax": exp z; "none": not read); src_valid [N,1,H,W]: zero
    leaves the source out.  Returns (results [N + 1, K] float64 on the device: one row per sample and the totals row, columns
    evaluate.FLOW_SPLAT_COLUMNS; out [N,C,H,W], weight [N,1,H,W], hole [N,1,H,W], status uint8 [N,1,H,W]: each None where not asked for)."""
    (v, f, z, m), (N, Cc, H, W) = _flow_splat_blobs("flow_splat_forward", values, flow, metric, src_valid)
    imp = _flow_splat_importance("flow_splat_forward", importance)
    dev = v.device
    ws = torch.empty(flow_splat_sizes(N, Cc, H, W)[0], dtype=torch.uint8, device=dev)
    results = torch.empty((N + 1, _FLOW_SPLAT_K), dtype=torch.float64, device=dev)
    new = lambda want, ch, dtype=torch.float32: torch.empty((N, ch, H, W), dtype=dtype, device=dev) if want else None
    o, w, h, s = new(out, Cc), new(weight, 1), new(hole, 1), new(status, 1, torch.uint8)
    check(_lib.lib().fn2_flow_splat_forward(_ptr(v), _ptr(f), _ptr(z), _ptr(m), N, Cc, H, W, C.c_float(float(t)), imp, int(bool(normalize)),
                                            int(fill_value), _ptr(results), _ptr(o), _ptr(w), _ptr(h), _ptr(s), _ptr(ws), ws.numel(),
                                            _stream()))
    return results, o, w, h, s


def flow_splat_backward(out_diff, weight_diff, values, flow, metric, src_valid, out, weight, t=1.0, importance="none", normalize=False,
                        need_values=True, need_flow=True, need_metric=True):
    """The gradients of flow_splat_forward's out (times out_diff) and weight (times weight_diff, or None) for values, flow and metric; out,
    weight: what the forward returned for the same inputs (out may be None where normalize is off).  Returns (values_diff, flow_diff,
    metric_diff), each None where not asked for; metric_diff is None with importance "none"."""
    (v, f, z, m), (N, Cc, H, W) = _flow_splat_blobs("flow_splat_backward", values, flow, metric, src_valid)
    imp = _flow_splat_importance("flow_splat_backward", importance)
    dev = v.device
    g, gw, o, w = _chk(out_diff, "out_diff"), _chk_opt(weight_diff, "weight_diff"), _chk_opt(out, "out"), _chk(weight, "weight")
    for name, t_, ch in (("out_diff", g, Cc), ("weight_diff", gw, 1), ("out", o, Cc), ("weight", w, 1)):
        if t_ is not None and (tuple(t_.shape) != (N, ch, H, W) or t_.device != dev):
            raise ValueError(f"flow_splat_backward: {name} {tuple(t_.shape)} must be [{N},{ch},{H},{W}] on {dev}")
    new = lambda want, ch: torch.empty((N, ch, H, W), dtype=torch.float32, device=dev) if want else None
    dv, df, dz = new(need_values, Cc), new(need_flow, 2), new(need_metric and imp != 0 and z is not None, 1)
    check(_lib.lib().fn2_flow_splat_backward(_ptr(g), _ptr(gw), _ptr(v), _ptr(f), _ptr(z), _ptr(m), _ptr(o), _ptr(w), N, Cc, H, W,
                                             C.c_float(float(t)), imp, int(bool(normalize)), _ptr(dv), _ptr(df), _ptr(dz), _stream()))
    return dv, df, dz


_FLOW_TRACK_K =_lib.FLOW_TRACK_CONSTANTS["FN2_FLOW_TRACK_K"]      # columns of a results row (evaluate.TRACK_COLUMNS)


def flow_track_sizes(N: int, T: int, H: int, W: int, P: int):
    """(workspace bytes, K) of fn2_flow_track / fn2_flow_track_reseed for [N,T,2,H,W] flows and P points (include/flownet2_hip_flow_track.h)."""
    nbytes, k = C.c_size_t(), C.c_int()
    check(_lib.lib().fn2_flow_track_sizes(int(N), int(T), int(H), int(W), int(P), C.byref(nbytes), C.byref(k)))
    return nbytes.value, k.value


def _chk_bytes(t, name: str, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA (HIP) tensor; flownet2_amd has no CPU path")
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected uint8 {list(shape)}, got {t.dtype} {list(t.shape)}")
    return t.contiguous()


def flow_track(fw, bw, points, state=None, stop=None, stop_mask=8, alpha=(0.01, 0.5), tracks=True, steps=True):
    """Point trajectories (csrc/flow_track.hip) through fw, bw [N,T,2,H,W] from points [N,2,P] (a dense grid: [N,2,H,W]); state uint8 [N,P]
    or None, stop uint8 [N,T,1,H,W] or None.  Returns (results [N + 1, K] float64 on the device, columns evaluate.TRACK_COLUMNS; tracks
    [N,T+1,2,P] or None; points_out [N,2,P]; state_out uint8 [N,P]; steps int32 [N,P] or None)."""
    f, b = _chk(fw, "fw", 5), _chk(bw, "bw", 5)
    if f.shape != b.shape or f.shape[2] != 2:
        raise ValueError(f"flow_track: fw {tuple(f.shape)} and bw {tuple(b.shape)} must both be [N,T,2,H,W]")
    N, T, _, H, W = f.shape
    p = _chk(points, "points", None)
    if p.dim() < 3 or p.shape[0] != N or p.shape[1] != 2:
        raise ValueError(f"flow_track: points {tuple(p.shape)} must be [{N},2,P]")
    if f.device != b.device or f.device != p.device:
        raise ValueError(f"flow_track: fw on {f.device}, bw on {b.device}, points on {p.device}")
    P = p[0, 0].numel()
    s_in = _chk_bytes(state, "state", (N, P)) if state is not None else None
    s_map = _chk_bytes(stop, "stop", (N, T, 1, H, W)) if stop is not None else None
    ws = torch.empty(flow_track_sizes(N, T, H, W, P)[0], dtype=torch.uint8, device=f.device)
    results = torch.empty((N + 1, _FLOW_TRACK_K), dtype=torch.float64, device=f.device)
    tr = torch.empty((N, T + 1, 2, P), dtype=torch.float32, device=f.device) if tracks else None
    p_out = torch.empty((N, 2, P), dtype=torch.float32, device=f.device)
    s_out = torch.empty((N, P), dtype=torch.uint8, device=f.device)
    st = torch.empty((N, P), dtype=torch.int32, device=f.device) if steps else None
    check(_lib.lib().fn2_flow_track(_ptr(f), _ptr(b), _ptr(s_map), int(stop_mask), _ptr(p), _ptr(s_in), N, T, H, W, P, C.c_float(float(alpha[0])),
                                    C.c_float(float(alpha[1])), _ptr(results), _ptr(tr), _ptr(p_out), _ptr(s_out),
                                    C.cast(_ptr(st), C.POINTER(C.c_int)), _ptr(ws), ws.numel(), _stream()))
    return results, tr, p_out, s_out, st


def flow_track_reseed(points, state, size, cell, born=True):
    """fn2_flow_track_reseed on points [N,2,P] and state uint8 [N,P], IN PLACE, for a plane size = (H, W) cut into cells of `cell` pixels
    (P = ceil(H / cell) ceil(W / cell)): every stopped slot whose home cell no alive point covers starts anew at the cell's centre.
    Returns born uint8 [N,P] (or None)."""
    H, W = int(size[0]), int(size[1])
    cell = int(cell)
    if cell < 1 or H < 1 or W < 1:
        raise ValueError(f"flow_track_reseed: bad size ({H}, {W}) or cell {cell}")
    P = -(-H // cell) * -(-W // cell)
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise ValueError("points: expected a CUDA (HIP) tensor; flownet2_amd has no CPU path")
    N = points.shape[0]
    if points.dtype != torch.float32 or tuple(points.shape) != (N, 2, P) or not points.is_contiguous():
        raise ValueError(f"flow_track_reseed: points must be contiguous float32 [N,2,{P}] for size ({H}, {W}) and cell {cell}, got {tuple(points.shape)}")
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or tuple(state.shape) != (N, P) or not state.is_contiguous() \
            or state.device != points.device:
        raise ValueError(f"flow_track_reseed: state must be contiguous uint8 [{N},{P}] on {points.device}")
    ws = torch.empty(max(N * P, 1), dtype=torch.uint8, device=points.device)
    b = torch.empty((N, P), dtype=torch.uint8, device=points.device) if born else None
    check(_lib.lib().fn2_flow_track_reseed(_ptr(points), _ptr(state), _ptr(b), N, H, W, cell, _ptr(ws), ws.numel(), _stream()))
    return b


_FLOW_COLOR_NORMS = {n[len("FN2_FLOW_COLOR_NORM_"):].lower(): v for n, v in _lib.FLOW_VISUALIZE_CONSTANTS.items()}      # sample, batch, fixed


def flow_visualize_sizes(N: int, H: int, W: int):
    """Workspace bytes of fn2_flow_color for [N,2,H,W] (include/flownet2_hip_flow_visualize.h)."""
    nbytes = C.c_size_t()
    check(_lib.lib().fn2_flow_visualize_sizes(int(N), int(H), int(W), C.byref(nbytes)))
    return nbytes.value


def flow_color(flow, norm="sample", max_flow=None, maxrad=False):
    """Middlebury colour coding (csrc/flow_visualize.hip) of flow [N,2,H,W] -> (uint8 [N,H,W,3] on the device; the float [N] of the
    radius each sample was normalised by, or None).  norm: sample | batch | fixed, the last with max_flow > 0."""
    f = _chk(flow, "flow")
    if f.shape[1] != 2:
        raise ValueError(f"flow_color: flow {tuple(f.shape)} must be [N,2,H,W]")
    if norm not in _FLOW_COLOR_NORMS:
        raise ValueError(f"flow_color: norm must be one of {sorted(_FLOW_COLOR_NORMS)}, got {norm!r}")
    fixed = norm == "fixed"
    if fixed and max_flow is None:
        raise ValueError("flow_color: norm='fixed' needs max_flow")
    N, _, H, W = f.shape
    ws = None if fixed else torch.empty(flow_visualize_sizes(N, H, W), dtype=torch.uint8, device=f.device)
    rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=f.device)
    used = torch.empty((N,), dtype=torch.float32, device=f.device) if maxrad else None
    check(_lib.lib().fn2_flow_color(_ptr(f), N, H, W, _FLOW_COLOR_NORMS[norm], C.c_float(float(max_flow) if fixed else 0.0), _ptr(rgb), _ptr(used),
                                    _ptr(ws), ws.numel() if ws is not None else 0, _stream()))
    return rgb, used


def flow_error_map(pred, gt, valid=None, occ=None, abs_thresh=3.0, rel_thresh=0.05):
    """KITTI-style error image (csrc/flow_visualize.hip) of pred against gt [N,2,H,W]; valid / occ [N,1,H,W] or None -> uint8 [N,H,W,3]
    on the device."""
    p, g = _chk(pred, "pred"), _chk(gt, "gt")
    if p.shape != g.shape or p.shape[1] != 2:
        raise ValueError(f"flow_error_map: pred {tuple(p.shape)} and gt {tuple(g.shape)} must both be [N,2,H,W]")
    if p.device != g.device:
        raise ValueError(f"flow_error_map: pred on {p.device}, gt on {g.device}")
    N, _, H, W = p.shape
    v, o = _chk_opt(valid, "valid"), _chk_opt(occ, "occ")
    for name, m in (("valid", v), ("occ", o)):
        if m is not None and tuple(m.shape) != (N, 1, H, W):
            raise ValueError(f"flow_error_map: {name} {tuple(m.shape)} must be [{N},1,{H},{W}]")
    rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=p.device)
    check(_lib.lib().fn2_flow_error_map(_ptr(p), _ptr(g), _ptr(v), _ptr(o), N, H, W, C.c_float(float(abs_thresh)), C.c_float(float(rel_thresh)),
                                        _ptr(rgb), _stream()))
    return rgb


def channel_norm_forward(x):
    x = _chk(x, "bottom[0]")
    N, Cc, H, W = x.shape
    out = torch.empty((N, 1, H, W), device=x.device, dtype=torch.float32)
    check(_lib.lib().fn2_channel_norm_forward(_ptr(x), _ptr(out), N, Cc, H, W, _stream()))
    return out


def channel_norm_forward_slices(x, minus=None, out=None):
    """ChannelNorm(x - minus) (minus optional) over channel slices (blob, c0, C); out = (blob, c0, 1) or None for a new [N,1,H,W] blob."""
    b, bctot, bc0, Cc = _as_slice(x, "bottom[0]")
    N, _, H, W = b.shape
    m, mctot, mc0 = None, 0, 0
    if minus is not None:
        m, mctot, mc0, Cm = _as_slice(minus, "bottom[1]")
        if Cm != Cc or tuple(m.shape[2:]) != (H, W) or m.shape[0] != N:
            raise ValueError("channel_norm: the subtrahend does not match the bottom")
    if out is None:
        out = torch.empty((N, 1, H, W), device=b.device, dtype=torch.float32)
    top, tctot, tc0, Ct = _as_slice(out, "top[0]")
    if Ct != 1 or top.shape[0] != N or tuple(top.shape[2:]) != (H, W):
        raise ValueError("channel_norm: top slice must be one channel of the bottom's size")
    check(_lib.lib().fn2_channel_norm_forward_slices(_ptr(b), bctot, bc0, _ptr(m), mctot, mc0, _ptr(top), tctot, tc0, N, Cc, H, W, _stream()))
    return top


def channel_norm_backward(x, top, top_diff):
    x, top, td = _chk(x, "bottom[0]"), _chk(top, "top"), _chk(top_diff, "top.diff")
    N, Cc, H, W = x.shape
    d = torch.empty_like(x)
    check(_lib.lib().fn2_channel_norm_backward(_ptr(x), _ptr(top), _ptr(td), _ptr(d), N, Cc, H, W, _stream()))
    return d


def downsample_forward(x, top_height, top_width):
    x = _chk(x, "bottom[0]")
    N, Cc, H, W = x.shape
    if top_height < 1 or top_width < 1:
        raise ValueError("DownsampleLayer must have top_height > 0 and top_width > 0")
    out = torch.empty((N, Cc, int(top_height), int(top_width)), device=x.device, dtype=torch.float32)
    check(_lib.lib().fn2_downsample_forward(_ptr(x), _ptr(out), N, Cc, H, W, int(top_height), int(top_width), _stream()))
    return out


def downsample_forward_multi(x, sizes):
    """Downsample(x) to every (height, width) of `sizes` in ONE launch (fn2_downsample_forward_multi: up to 8 tops, each at least 2 x 2 and of
    another size than x); the bits of downsample_forward per size."""
    x = _chk(x, "bottom[0]")
    N, Cc, H, W = x.shape
    sizes = [(int(h), int(w)) for h, w in sizes]
    outs = [torch.empty((N, Cc, h, w), device=x.device, dtype=torch.float32) for h, w in sizes]
    n = len(sizes)
    ptrs = (C.c_void_p * n)(*[_ptr(o) for o in outs])
    hs, ws = (C.c_int * n)(*[h for h, _ in sizes]), (C.c_int * n)(*[w for _, w in sizes])
    check(_lib.lib().fn2_downsample_forward_multi(_ptr(x), ptrs, hs, ws, n, N, Cc, H, W, _stream()))
    return outs


def downsample_multi_supported(x_shape, sizes) -> bool:
    H, W = int(x_shape[2]), int(x_shape[3])
    return 1 <= len(sizes) <= 8 and all(int(h) >= 2 and int(w) >= 2 and (int(h), int(w)) != (H, W) for h, w in sizes)


def predict_flow_conv_forward(x, weight, bias=None):
    """Convolution{kernel 3, stride 1, pad 1, num_output 2} (the FlowNet predict_flow heads)."""
    x, w = _chk(x, "bottom[0]"), _chk(weight, "weight")
    N, Cc, H, W = x.shape
    if tuple(w.shape) != (2, Cc, 3, 3):
        raise ValueError(f"predict_flow weight must be [2,{Cc},3,3], got {tuple(w.shape)}")
    b = _chk(bias, "bias", ndim=1) if bias is not None else None
    out = torch.empty((N, 2, H, W), device=x.device, dtype=torch.float32)
    nbytes = _lib.lib().fn2_predict_flow_conv_workspace_bytes(N, Cc, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    check(_lib.lib().fn2_predict_flow_conv_forward(_ptr(x), _ptr(w), _ptr(b), _ptr(out), N, Cc, H, W, _ptr(ws), nbytes, _stream()))
    return out


def upsample_flow_deconv_forward(x, weight, bias=None, out=None, out_c0=0):
    """Deconvolution{kernel 4, stride 2, pad 1, num_output 2} on a 2-channel flow (the upsample_flow heads); with `out` the two
    channels go to out[:, out_c0:out_c0+2] of a wider blob (the refinement Concat)."""
    x, w = _chk(x, "bottom[0]"), _chk(weight, "weight")
    N, Cc, H, W = x.shape
    if Cc != 2 or tuple(w.shape) != (2, 2, 4, 4):
        raise ValueError("upsample_flow expects a 2-channel flow and a [2,2,4,4] weight")
    b = _chk(bias, "bias", ndim=1) if bias is not None else None
    if out is not None:
        _chk(out, "top[0]")
        if out.shape[0] != N or tuple(out.shape[2:]) != (2 * H, 2 * W):
            raise ValueError(f"upsample_flow: top blob {tuple(out.shape)} does not match [{N},*,{2 * H},{2 * W}]")
        check(_lib.lib().fn2_upsample_flow_deconv_forward_into(_ptr(x), _ptr(w), _ptr(b), _ptr(out), N, H, W, out.shape[1], int(out_c0), _stream()))
        return out[:, out_c0:out_c0 + 2]
    out = torch.empty((N, 2, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
    check(_lib.lib().fn2_upsample_flow_deconv_forward(_ptr(x), _ptr(w), _ptr(b), _ptr(out), N, H, W, _stream()))
    return out


def predict_upsample_flow_forward(x, weight, bias, up_weight, up_bias, out, out_c0):
    """predict_flow_conv_forward(x) and upsample_flow_deconv_forward of it into out[:, out_c0:out_c0+2], the gather and the up-sampling
    in one launch (same bits).  Returns the flow [N,2,H,W], or None where the one-launch form declines the geometry."""
    x, w, uw = _chk(x, "bottom[0]"), _chk(weight, "weight"), _chk(up_weight, "upsample weight")
    N, Cc, H, W = x.shape
    if tuple(w.shape) != (2, Cc, 3, 3) or tuple(uw.shape) != (2, 2, 4, 4):
        raise ValueError(f"predict_upsample_flow: weights must be [2,{Cc},3,3] and [2,2,4,4], got {tuple(w.shape)} and {tuple(uw.shape)}")
    _chk(out, "top[0]")
    if out.shape[0] != N or tuple(out.shape[2:]) != (2 * H, 2 * W):
        raise ValueError(f"predict_upsample_flow: top blob {tuple(out.shape)} does not match [{N},*,{2 * H},{2 * W}]")
    if not _lib.lib().fn2_predict_upsample_flow_supported(N, Cc, H, W):
        return None
    b = _chk(bias, "bias", ndim=1) if bias is not None else None
    ub = _chk(up_bias, "upsample bias", ndim=1) if up_bias is not None else None
    flow = torch.empty((N, 2, H, W), device=x.device, dtype=torch.float32)
    nbytes = _lib.lib().fn2_predict_flow_conv_workspace_bytes(N, Cc, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    check(_lib.lib().fn2_predict_upsample_flow_forward_into(_ptr(x), _ptr(w), _ptr(b), _ptr(flow), _ptr(uw), _ptr(ub), _ptr(out), N, Cc, H, W,
                                                            out.shape[1], int(out_c0), _ptr(ws), nbytes, _stream()))
    return flow


def bias_leaky_relu_(x, bias=None, negative_slope=0.1):
    """In place: x[n,c] = leaky_relu(x[n,c] + bias[c]) -- the bias term + ReLU layer that follow every FlowNet conv/deconv."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("bias_leaky_relu_: expected a contiguous float32 CUDA (HIP) NCHW tensor")
    N, Cc, H, W = x.shape
    b = _chk_opt(bias, "bias", 1)
    if b is not None and b.numel() != Cc:
        raise ValueError(f"bias must have {Cc} entries, got {b.numel()}")
    check(_lib.lib().fn2_bias_leaky_relu_forward(_ptr(x), _ptr(b), N, Cc, H, W, C.c_float(float(negative_slope)), _stream()))
    return x


def scale_shift_forward(x, scale, shift=None, out=None, out_c0=0):
    """out[:, out_c0 : out_c0 + C] = x * scale + shift[c] with the product and the sum rounded separately (csrc/bias_act.hip): the deploy
    head's Eltwise{1/255} + mean subtraction in one pass, written into a channel slice of `out` [N, *, H, W] (a new blob if None)."""
    x = _chk(x, "bottom[0]")
    N, Cc, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk(out, "top[0]")
        if out.shape[0] != N or tuple(out.shape[2:]) != (H, W):
            raise ValueError("scale_shift: top blob does not match the bottom")
    s = _chk_opt(shift, "shift", 1)
    check(_lib.lib().fn2_scale_shift_forward(_ptr(x), _ptr(out), _ptr(s), N, Cc, H, W, out.shape[1], out_c0, C.c_float(float(scale)), _stream()))
    return out


def predict_flow_conv_backward_supported(N, C, H, W) -> bool:
    return bool(_lib.lib().fn2_predict_flow_conv_backward_supported(int(N), int(C), int(H), int(W)))


def _head_diffs(what, out, needs, shapes, device):
    """The (bottom_diff, weight_diff, bias_diff) blobs of a flow head's backward: new ones, or those of `out` (a triple, None where the
    gradient is not needed), checked against their shapes."""
    if out is None:
        return tuple(torch.empty(s, device=device, dtype=torch.float32) if need else None for need, s in zip(needs, shapes))
    if len(out) != 3:
        raise ValueError(what + ": out must be (bottom_diff, weight_diff, bias_diff)")
    for t, need, s, name in zip(out, needs, shapes, ("bottom.diff", "weight.diff", "bias.diff")):
        if (t is not None) != bool(need):
            raise ValueError(f"{what}: out holds a {name} exactly where that gradient is needed")
        if t is not None and (_chk(t, name, ndim=len(s)) is not t or tuple(t.shape) != tuple(s)):
            raise ValueError(f"{what}: {name} must be a contiguous {list(s)} blob")
    return tuple(out)


def predict_flow_conv_backward(x, weight, top_diff, need_x=True, need_w=True, need_b=True, out=None, accumulate=False):
    """Backward of predict_flow (Convolution{3,1,1} C -> 2): (bottom_diff, weight_diff, bias_diff), None where not needed.  `x` may be a
    channel slice (blob, c0, C).  `out` = the three gradient blobs to write (None where not needed); with `accumulate` the weight and
    bias gradients are added to what `out` holds (the bottom gradient is always overwritten)."""
    xb, xctot, xc0, Cc = _as_slice(x, "bottom[0]")
    w, g = _chk(weight, "weight"), _chk(top_diff, "top.diff")
    N, _, H, W = xb.shape
    if tuple(w.shape) != (2, Cc, 3, 3) or tuple(g.shape) != (N, 2, H, W):
        raise ValueError("predict_flow_conv_backward: weight must be [2,C,3,3] and top_diff [N,2,H,W]")
    if accumulate and out is None:
        raise ValueError("predict_flow_conv_backward: accumulate needs the gradients to add to (out)")
    dx, dw, db = _head_diffs("predict_flow_conv_backward", out, (need_x, need_w, need_b), ((N, Cc, H, W), tuple(w.shape), (2,)), g.device)
    nbytes = _lib.lib().fn2_predict_flow_conv_backward_workspace_bytes(N, Cc, H, W) if (need_w or need_b) else 0
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=g.device)
    check(_lib.lib().fn2_predict_flow_conv_backward(_ptr(xb), xctot, xc0, _ptr(w), _ptr(g), _ptr(dx), _ptr(dw), _ptr(db), N, Cc, H, W,
                                                    int(bool(accumulate)), _ptr(ws), nbytes, _stream()))
    return dx, dw, db


def upsample_flow_deconv_backward(x, weight, top_diff, need_x=True, need_w=True, need_b=True, out=None, accumulate=False):
    """Backward of upsample_flow (Deconvolution{4,2,1} 2 -> 2): (bottom_diff, weight_diff, bias_diff), None where not needed; `out` and
    `accumulate` as for predict_flow_conv_backward."""
    x, w, g = _chk(x, "bottom[0]"), _chk(weight, "weight"), _chk(top_diff, "top.diff")
    N, Cc, H, W = x.shape
    if Cc != 2 or tuple(w.shape) != (2, 2, 4, 4) or tuple(g.shape) != (N, 2, 2 * H, 2 * W):
        raise ValueError("upsample_flow_deconv_backward: bottom [N,2,H,W], weight [2,2,4,4], top_diff [N,2,2H,2W]")
    if accumulate and out is None:
        raise ValueError("upsample_flow_deconv_backward: accumulate needs the gradients to add to (out)")
    dx, dw, db = _head_diffs("upsample_flow_deconv_backward", out, (need_x, need_w, need_b), (tuple(x.shape), (2, 2, 4, 4), (2,)), g.device)
    nbytes = _lib.lib().fn2_upsample_flow_deconv_backward_workspace_bytes(N, H, W) if (need_w or need_b) else 0
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=g.device)
    check(_lib.lib().fn2_upsample_flow_deconv_backward(_ptr(x), _ptr(w), _ptr(g), _ptr(dx), _ptr(dw), _ptr(db), N, H, W, int(bool(accumulate)),
                                                       _ptr(ws), nbytes, _stream()))
    return dx, dw, db


def conv_k7s2_relu_supported(Cin, Hin, Win, Cout) -> bool:
    return bool(_lib.lib().fn2_conv_k7s2_relu_supported(int(Cin), int(Hin), int(Win), int(Cout)))


def conv_k7s2_wgrad_supported(N, Cin, Hin, Win, Cout) -> bool:
    return bool(_lib.lib().fn2_conv_k7s2_wgrad_supported(int(N), int(Cin), int(Hin), int(Win), int(Cout)))


def conv_k7s2_wgrad_ksplit(N, Cin, Hin, Win, Cout) -> int:
    return int(_lib.lib().fn2_conv_k7s2_wgrad_ksplit(int(N), int(Cin), int(Hin), int(Win), int(Cout)))


def conv_k7s2_wgrad(top_diff, bottom):
    """weight_diff [Cout, Cin, 7, 7] of the 7x7 / 2 / 3 stem convolution (csrc/conv_stem_wgrad.hip); top_diff [N, 64, Ho, Wo], bottom [N, Cin, H, W]."""
    d, x = _chk(top_diff, "top.diff"), _chk(bottom, "bottom[0]")
    N, Cin, H, W = x.shape
    Cout = d.shape[1]
    if tuple(d.shape) != (N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise ValueError(f"conv_k7s2_wgrad: top_diff {tuple(d.shape)} does not belong to a bottom of {tuple(x.shape)}")
    dw = torch.empty((Cout, Cin, 7, 7), device=x.device, dtype=torch.float32)
    ws, need = _scratch(x.device, _lib.lib().fn2_conv_k7s2_wgrad_workspace_bytes(N, Cin, H, W, Cout))
    check(_lib.lib().fn2_conv_k7s2_wgrad(_ptr(d), _ptr(x), _ptr(dw), N, Cin, H, W, Cout, 0, _ptr(ws), need, _stream()))
    return dw


def conv_k7s2_relu_forward(x, weight, bias=None, negative_slope=0.1):
    """leaky_relu(Convolution{kernel 7, stride 2, pad 3}(x) + bias): conv1 + ReLU1 of the FlowNet encoders, one kernel."""
    x, w = _chk(x, "bottom[0]"), _chk(weight, "weight")
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    if tuple(w.shape) != (Cout, Cin, 7, 7):
        raise ValueError(f"stem weight must be [Cout,{Cin},7,7], got {tuple(w.shape)}")
    b = _chk_opt(bias, "bias", 1)
    out = torch.empty((N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1), device=x.device, dtype=torch.float32)
    check(_lib.lib().fn2_conv_k7s2_relu_forward(_ptr(x), _ptr(w), _ptr(b), _ptr(out), N, Cin, H, W, Cout,
                                                C.c_float(float(negative_slope)), _stream()))
    return out


CONV_ROUTE_NONE, CONV_ROUTE_DIRECT, CONV_ROUTE_WINOGRAD, CONV_ROUTE_PLANE, CONV_ROUTE_STEM, CONV_ROUTE_HEAD = _consts(
    "CONV_ROUTE_NONE", "CONV_ROUTE_DIRECT", "CONV_ROUTE_WINOGRAD", "CONV_ROUTE_PLANE", "CONV_ROUTE_STEM", "CONV_ROUTE_HEAD")
DECONV_ROUTE_NONE, DECONV_ROUTE_GEMM, DECONV_ROUTE_PLANE, DECONV_ROUTE_HEAD = _consts("DECONV_ROUTE_NONE", "DECONV_ROUTE_GEMM", "DECONV_ROUTE_PLANE",
                                                                                      "DECONV_ROUTE_HEAD")
ROUTE_FORCE, ROUTE_BF16X3, ROUTE_WINO_BF16X3 = _consts("ROUTE_FORCE", "ROUTE_BF16X3", "ROUTE_WINO_BF16X3")          # flags of fn2_conv_route
CONV_ARITH_BF16X3, = _consts("CONV_ARITH_BF16X3")         # split-bf16 arithmetic, a bit beside CONV_ROUTE_DIRECT / CONV_ROUTE_WINOGRAD in the route value (not a route)
CONV_FWD_ROUTES = {0: None, 1: "direct", 2: "wino", 3: "plane", 4: "stem", 5: "head"}
DECONV_FWD_ROUTES = {0: None, 1: "gemm", 2: "plane", 3: "head"}
CONV_ROUTES = {0: None, 1: "direct", 2: "wino", 3: "plane", 4: None, 5: None}     # conv_route(): the three general families only (4 / 5: stem / flow head)
DECONV_ROUTES = {0: None, 1: "gemm", 2: "plane", 3: None}      # 3: the 2-channel upsample_flow head (upsample_flow_deconv)


def conv_route(N, Cin, Hin, Win, Cout, kernel, stride, pad, force=False):
    """Which kernel family the LIBRARY picks for Convolution{kernel, stride, pad} Cin -> Cout on [N, Cin, Hin, Win] (fn2_conv_route,
    csrc/conv_route.cpp -- the same decision the Caffe adapter gets): "wino", "plane", "direct" or None."""
    return CONV_ROUTES[conv_forward_route(conv_desc(N, Cin, Hin, Win, Cout, kernel, stride, pad), force)]


def deconv_route(N, Cin, Hin, Win, Cout, kernel=4, stride=2, pad=1):
    """fn2_deconv_route: "gemm" (weight^T x bottom on the 1x1 kernel + col2im), "plane" (parity classes, small maps) or None."""
    return DECONV_ROUTES[deconv_forward_route(conv_desc(N, Cin, Hin, Win, Cout, kernel, stride, pad))]


BWD_ROUTES = {0: None, 1: "wino", 2: "tconv", 3: "plane", 4: "direct", 5: "deconv_plane"}


def conv_desc(N, Cin, Hin, Win, Cout, kernel, stride, pad):
    """fn2_conv_desc: bottom [N, Cin, Hin, Win] of a Convolution{kernel, stride, pad} (Cin -> Cout) or of a Deconvolution{4, 2, 1}."""
    return _lib.ConvDesc(int(N), int(Cin), int(Hin), int(Win), int(Cout), int(kernel), int(stride), int(pad))


def conv_forward_route(desc, force=False, bf16x3=False, wino_bf16x3=False) -> int:
    """Which own kernel serves the forward pass of this Convolution (fn2_conv_route; 0 = none, names: CONV_FWD_ROUTES).  bf16x3: the layers
    the split-bf16 kernel takes come back as CONV_ROUTE_DIRECT | CONV_ARITH_BF16X3, every other layer as without it; wino_bf16x3, a flag of
    its own: the Winograd layers the split-bf16 Winograd kernel takes (csrc/conv_wino_bf16x3.hip) come back as CONV_ROUTE_WINOGRAD |
    CONV_ARITH_BF16X3.  conv_pack_weights and conv_forward take these values as they are."""
    flags = (ROUTE_FORCE if force else 0) | (ROUTE_BF16X3 if bf16x3 else 0) | (ROUTE_WINO_BF16X3 if wino_bf16x3 else 0)
    return int(_lib.lib().fn2_conv_route(C.byref(desc), flags))


def deconv_forward_route(desc, bf16x3=False) -> int:
    """Which own kernel serves the forward pass of this Deconvolution{4, 2, 1} (fn2_deconv_route; 0 = none, names: DECONV_FWD_ROUTES).
    bf16x3: the layers of the GEMM route that the split-bf16 GEMM takes come back as DECONV_ROUTE_GEMM | CONV_ARITH_BF16X3, every other layer
    as without it; conv_pack_weights and conv_forward (transposed=True) take that value as it is."""
    return int(_lib.lib().fn2_deconv_route(C.byref(desc), ROUTE_BF16X3 if bf16x3 else 0))


def conv_pack_weights(weight, desc, route, transposed=False):
    """The layer's weight blob ([Cout, Cin, k, k]; Deconvolution: [Cin, Cout, 4, 4]) -> the operand its forward kernel reads
    (fn2_conv_pack_weights / fn2_deconv_pack_weights: once per weight update)."""
    w = _chk(weight, "weight")
    L = _lib.lib()
    floats, pack = (L.fn2_deconv_packed_weight_floats, L.fn2_deconv_pack_weights) if transposed else (L.fn2_conv_packed_weight_floats, L.fn2_conv_pack_weights)
    n = int(floats(C.byref(desc), int(route)))
    k = desc.kernel
    if n == 0 or tuple(w.shape) != ((desc.Cin, desc.Cout, k, k) if transposed else (desc.Cout, desc.Cin, k, k)):
        raise ValueError("conv_pack_weights: route %d has no operand for a weight of shape %s" % (route, tuple(w.shape)))
    packed = torch.empty(n, device=w.device, dtype=torch.float32)
    check(pack(C.byref(desc), int(route), _ptr(w), _ptr(packed), _stream()))
    return packed


def conv_forward(x, packed, bias, desc, route, transposed=False, relu=True, negative_slope=0.1, out=None, out_c0=0, in_c0=0):
    """act(Convolution(x[:, in_c0:in_c0+Cin]) + bias) -> out[:, out_c0:out_c0+Cout] (a new blob if out is None) on the kernel `route` names
    (fn2_conv_forward; transposed: the Deconvolution{4, 2, 1}, top 2H x 2W, fn2_deconv_forward).  packed = conv_pack_weights(weight, desc,
    route, transposed).  Returns the top blob."""
    x = _chk(x, "bottom[0]")
    N, Ctot, H, W = x.shape
    k, s, p = desc.kernel, desc.stride, desc.pad
    if (N, H, W) != (desc.N, desc.Hin, desc.Win) or in_c0 < 0 or in_c0 + desc.Cin > Ctot:
        raise ValueError(f"conv_forward: bottom blob {tuple(x.shape)} does not hold the layer's [{desc.N},{desc.Cin},{desc.Hin},{desc.Win}] at channel {in_c0}")
    Ho, Wo = (2 * H, 2 * W) if transposed else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    if out is None:
        out = torch.empty((N, desc.Cout, Ho, Wo), device=x.device, dtype=torch.float32)
    else:
        _chk(out, "top[0]")
        if not out.is_contiguous() or out.shape[0] != N or tuple(out.shape[2:]) != (Ho, Wo) or out_c0 < 0 or out_c0 + desc.Cout > out.shape[1]:
            raise ValueError(f"conv_forward: top blob {tuple(out.shape)} does not match [{N},>={out_c0 + desc.Cout},{Ho},{Wo}]")
    b = _chk(bias, "bias", ndim=1) if bias is not None else None
    pw = _chk(packed, "packed weight", ndim=None)
    L = _lib.lib()
    if pw.numel() != int((L.fn2_deconv_packed_weight_floats if transposed else L.fn2_conv_packed_weight_floats)(C.byref(desc), int(route))):
        raise ValueError("conv_forward: the operand has %d floats, not what route %d reads for this layer" % (pw.numel(), route))
    need = int((L.fn2_deconv_workspace_bytes if transposed else L.fn2_conv_workspace_bytes)(C.byref(desc), int(route)))
    if transposed and (route & ~CONV_ARITH_BF16X3) == DECONV_ROUTE_GEMM:
        # the column matrix lives for this call only (the per-stream scratch never shrinks: it would pin the largest one for good)
        ws = torch.empty((need + 3) // 4, device=x.device, dtype=torch.float32)
    else:
        ws = _plane_workspace(x.device, need) if need else None         # the K-split scratch of the small-map routes
    check((L.fn2_deconv_forward if transposed else L.fn2_conv_forward)(
        C.byref(desc), int(route), _ptr(x), Ctot, int(in_c0), _ptr(pw), _ptr(b), _ptr(out), out.shape[1], int(out_c0),
        int(bool(relu)), C.c_float(float(negative_slope)), _ptr(ws), need, _stream()))
    return out


def conv_backward_data_route(desc, transposed=False, bf16x3=False) -> int:
    """Which own kernel computes bottom_diff of this layer (fn2_conv_backward_data_route; 0 = none, names: BWD_ROUTES).  bf16x3: the layers
    the split-bf16 data-gradient kernel takes (csrc/tconv_bf16x3.hip: the 5x5 / 2 / 2 class of BWD_ROUTE_TCONV) come back as
    BWD_ROUTE_TCONV | CONV_ARITH_BF16X3, every other layer as without it (fn2_conv_backward_data_route_flags); the pack, run and masked
    wrappers below take that value."""
    return int(_lib.lib().fn2_conv_backward_data_route_flags(C.byref(desc), int(bool(transposed)), ROUTE_BF16X3 if bf16x3 else 0))


def _check_dgrad_operand(what, packed, desc, tr, route):
    """The operand must be the one packed for THIS route: the exact and the split-bf16 operand of a layer differ in size and layout."""
    n = int(_lib.lib().fn2_conv_backward_data_packed_weight_floats(C.byref(desc), tr, int(route)))
    if n == 0:
        raise ValueError("%s: route %d is not this layer's" % (what, route))
    if packed.numel() != n:
        raise ValueError("%s: the operand has %d floats, route %d of this layer needs %d (packed for another route?)" % (what, packed.numel(), route, n))


def conv_backward_data_pack_weights(weight, desc, transposed, route):
    """The layer's weight blob ([Cout, Cin, k, k]; Deconvolution: [Cin, Cout, 4, 4]) -> the operand its data-gradient kernel reads."""
    w = _chk(weight, "weight")
    L, tr = _lib.lib(), int(bool(transposed))
    n = int(L.fn2_conv_backward_data_packed_weight_floats(C.byref(desc), tr, int(route)))
    if n == 0:
        raise ValueError("conv_backward_data_pack_weights: route %d is not this layer's" % route)
    packed = torch.empty(n, device=w.device, dtype=torch.float32)
    need = int(L.fn2_conv_backward_data_pack_workspace_bytes(C.byref(desc), tr, int(route)))
    ws = torch.empty(need // 4, device=w.device, dtype=torch.float32) if need else None
    check(L.fn2_conv_backward_data_pack_weights(C.byref(desc), tr, int(route), _ptr(w), _ptr(packed), _ptr(ws), need, _stream()))
    return packed


def conv_backward_data(top_diff, packed_weight, desc, transposed, route, top_c0=0):
    """bottom_diff [N, Cin, Hin, Win] of the layer from top_diff (a blob, the layer's channels starting at top_c0).  The kernels compute
    channels in groups: the result is the leading-channel VIEW of a blob that has room for them (no copy)."""
    d = _chk(top_diff, "top_diff")
    L, tr = _lib.lib(), int(bool(transposed))
    Cp = int(L.fn2_conv_backward_data_computed_channels(C.byref(desc), tr, int(route)))
    if Cp == 0:
        raise ValueError("conv_backward_data: route %d is not this layer's" % route)
    _check_dgrad_operand("conv_backward_data", packed_weight, desc, tr, route)
    out = torch.empty((desc.N, Cp, desc.Hin, desc.Win), device=d.device, dtype=torch.float32)
    need = int(L.fn2_conv_backward_data_workspace_bytes_with_room(C.byref(desc), tr, int(route), Cp))      # (the blob has room: no padded copy in the scratch)
    ws = _plane_workspace(d.device, need) if need else None
    check(L.fn2_conv_backward_data(C.byref(desc), tr, int(route), _ptr(d), d.shape[1], int(top_c0), _ptr(packed_weight), _ptr(out), Cp, 0, Cp,
                                   _ptr(ws), need, _stream()))
    return out[:, :desc.Cin] if Cp != desc.Cin else out


def conv_backward_weights_supported(desc, transposed=False) -> bool:
    return bool(_lib.lib().fn2_conv_backward_weights_supported(C.byref(desc), int(bool(transposed))))


def conv_backward_weights_arith(desc, transposed=False, bf16x3=False) -> int:
    """Arithmetic of the layer's weight gradient (fn2_conv_backward_weights_arith): CONV_ARITH_BF16X3 where bf16x3 is asked for and the
    split-bf16 kernel takes the layer (csrc/conv_wgrad_bf16x3.hip: Convolution{5, 2, 2}), else 0 = the exact kernel."""
    return int(_lib.lib().fn2_conv_backward_weights_arith(C.byref(desc), int(bool(transposed)), ROUTE_BF16X3 if bf16x3 else 0))


def conv_backward_weights(bottom, top_diff, desc, transposed=False, out=None, accumulate=False, bottom_c0=0, top_c0=0, bf16x3=False):
    """weight_diff of the layer ([Cout, Cin, k, k]; Deconvolution: [Cin, Cout, 4, 4]) (+)= ... (fn2_conv_backward_weights: the stem kernel or
    csrc/conv_wgrad.hip, deterministic).  bf16x3: in split-bf16 arithmetic where conv_backward_weights_arith gives the layer to that kernel
    (fn2_conv_backward_weights_arith_run), exact everywhere else."""
    x, d = _chk(bottom, "bottom"), _chk(top_diff, "top_diff")
    L, tr = _lib.lib(), int(bool(transposed))
    k = desc.kernel
    shape = (desc.Cin, desc.Cout, k, k) if transposed else (desc.Cout, desc.Cin, k, k)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
        accumulate = False
    else:
        out = _chk(out, "weight diff")
        if tuple(out.shape) != shape:
            raise ValueError("conv_backward_weights: weight diff has the wrong shape")
    arith = conv_backward_weights_arith(desc, transposed, bf16x3)         # 0: the exact kernel, as fn2_conv_backward_weights runs it
    need = int(L.fn2_conv_backward_weights_workspace_bytes_arith(C.byref(desc), tr, arith))
    ws = _plane_workspace(x.device, need) if need else None
    check(L.fn2_conv_backward_weights_arith_run(C.byref(desc), tr, arith, _ptr(x), x.shape[1], int(bottom_c0), _ptr(d), d.shape[1], int(top_c0),
                                                _ptr(out), int(bool(accumulate)), _ptr(ws), need, _stream()))
    return out


def conv_backward_data_masked_supported(desc, transposed, route) -> bool:
    return bool(_lib.lib().fn2_conv_backward_data_masked_supported(C.byref(desc), int(bool(transposed)), int(route)))


def conv_backward_data_masked(top_diff, packed, desc, transposed, route, bottom_data, negative_slope, top_c0=0, data_c0=0):
    """bottom_diff = (weight^T x top_diff) * leaky_relu'(bottom_data): the data gradient with ReLUBackward of the layer in front folded into
    the kernel's epilogue (fn2_conv_backward_data_masked; the transposed-convolution route).  bottom_data = this layer's bottom blob, the
    activated output of the layer in front (may be a channel slice: data_c0)."""
    d, y = _chk(top_diff, "top_diff"), _chk(bottom_data, "bottom data")
    _check_dgrad_operand("conv_backward_data_masked", packed, desc, int(bool(transposed)), route)
    out = torch.empty((desc.N, desc.Cin, desc.Hin, desc.Win), device=d.device, dtype=torch.float32)
    check(_lib.lib().fn2_conv_backward_data_masked(C.byref(desc), int(bool(transposed)), int(route), _ptr(d), d.shape[1], int(top_c0), _ptr(packed),
                                                   _ptr(out), desc.Cin, 0, _ptr(y), y.shape[1], int(data_c0), C.c_float(float(negative_slope)), _stream()))
    return out


def conv_backward_weights_bias_fused(desc, transposed=False) -> bool:
    return bool(_lib.lib().fn2_conv_backward_weights_bias_fused(C.byref(desc), int(bool(transposed))))


def conv_backward_weights_bias(bottom, top_diff, desc, transposed=False, out=None):
    """(weight_diff, bias_diff) of a layer from one pass over top_diff (fn2_conv_backward_weights_bias: the stem kernel sums the operand it
    feeds to the matrix pipe).  `out`: write weight_diff there (a gradient-bucket slot)."""
    x, d = _chk(bottom, "bottom"), _chk(top_diff, "top_diff")
    L, tr = _lib.lib(), int(bool(transposed))
    k = desc.kernel
    dw = out if out is not None else torch.empty((desc.Cout, desc.Cin, k, k), device=x.device, dtype=torch.float32)
    db = torch.empty(desc.Cout, device=x.device, dtype=torch.float32)
    need = int(L.fn2_conv_backward_weights_workspace_bytes(C.byref(desc), tr))
    ws = _plane_workspace(x.device, need) if need else None
    check(L.fn2_conv_backward_weights_bias(C.byref(desc), tr, _ptr(x), _ptr(d), _ptr(dw), _ptr(db), 0, _ptr(ws), need, _stream()))
    return dw, db


def conv_backward_bias(top_diff, C_, top_c0=0, out=None, accumulate=False):
    """bias_diff[c] (+)= sum over n, y, x of top_diff[n, top_c0 + c] (backward_gpu_bias, base_conv_layer.cpp:389-393), fixed order."""
    d = _chk(top_diff, "top_diff")
    N, Ctot, H, W = d.shape
    if out is None:
        out = torch.empty(C_, device=d.device, dtype=torch.float32)
        accumulate = False
    need = int(_lib.lib().fn2_bias_leaky_relu_backward_workspace_bytes(N, C_, H, W))
    ws = _plane_workspace(d.device, need)
    check(_lib.lib().fn2_conv_backward_bias(_ptr(d), Ctot, int(top_c0), _ptr(out), N, int(C_), H, W, int(bool(accumulate)), _ptr(ws), need, _stream()))
    return out


class _ConvAbi:
    """The wrappers of the general-geometry kernels (csrc/conv_general.hip), written once over what differs between their three C ABIs:
    name = the public prefix (the C one is "fn2_" + name, the word after "conv_" tags the family's cached operands); axes = axes of its
    blobs; arg(g) = the geometry as C takes it; read(g) = (N, Cin, bottom size, Cout, kernel, group), sizes as tuples; key(g) = what of
    the geometry a packed operand depends on beside the weight; out_shape(g, transposed) (default: the ABI's C function); sep: between
    the numbers of a layer's extent in a message; shape_first: pack_weights checks the weight's shape before it asks C for the sizes."""

    def __init__(self, name, axes, arg, read, key=tuple, out_shape=None, sep=",", shape_first=False):
        self.name, self.axes, self.arg, self.read, self.key, self.sep, self.shape_first = name, axes, arg, read, key, sep, shape_first
        self.tag = name[len("conv_"):]
        self.out_shape = out_shape or self.c_out_shape
        self._c = {}

    def c(self, fn):
        """The ABI's C entry point `fn`, looked up once (a call of these wrappers is a few microseconds of host time)."""
        f = self._c.get(fn)
        if f is None:
            f = self._c[fn] = getattr(_lib.lib(), "fn2_%s_%s" % (self.name, fn))
        return f

    def supported(self, g, transposed=False):
        return bool(self.c("supported")(self.arg(g), int(bool(transposed))))

    def sizes(self, g, transposed=False):
        n = [C.c_size_t() for _ in range(4)]
        check(self.c("sizes")(self.arg(g), int(bool(transposed)), *(C.byref(v) for v in n)))
        return tuple(int(v.value) for v in n)

    def c_out_shape(self, g, transposed=False):
        n = [C.c_int() for _ in range(self.axes - 2)]
        check(self.c("out_shape")(self.arg(g), int(bool(transposed)), *[C.byref(v) for v in n]))
        return tuple([v.value for v in n])

    @staticmethod
    def weight_shape(layer, transposed):
        N, Cin, size, Cout, kernel, group = layer
        return ((Cin, Cout // group) if transposed else (Cout, Cin // group)) + kernel

    def blobs(self, what, g, transposed, bottom, bottom_c0, top, top_c0):
        """Check that the blobs given hold the layer's bottom and top slices; -> (read(g), top size)."""
        out = self.out_shape(g, transposed)
        layer = N, Cin, size, Cout, _, _ = self.read(g)
        for t, c0, Cc, ext, name in ((bottom, bottom_c0, Cin, size, "bottom"), (top, top_c0, Cout, out, "top")):
            if t is not None and (not t.is_contiguous() or (t.shape[0],) + tuple(t.shape[2:]) != (N,) + ext or c0 < 0 or c0 + Cc > t.shape[1]):
                layer = "[" + self.sep.join(str(v) for v in (N, Cc) + ext) + "]"
                raise ValueError(f"{what}: {name} blob {tuple(t.shape)} does not hold the layer's {layer} at channel {c0}")
        return layer, out

    def pack_weights(self, weight, g, transposed=False, backward=False):
        w = _chk(weight, "weight", ndim=self.axes)
        sizes = None if self.shape_first else self.sizes(g, transposed)
        if tuple(w.shape) != self.weight_shape(self.read(g), transposed):
            raise ValueError("%s_pack_weights: weight of shape %s is not this layer's" % (self.name, tuple(w.shape)))
        sizes = sizes or self.sizes(g, transposed)
        packed = torch.empty(sizes[1 if backward else 0], device=w.device, dtype=torch.float32)
        check(self.c("pack_weights")(self.arg(g), int(bool(transposed)), 1 if backward else 0, _ptr(w), _ptr(packed), _stream()))
        return packed

    def forward(self, x, packed, bias, g, transposed=False, relu=False, negative_slope=0.0, out=None, out_c0=0, in_c0=0):
        what = self.name + "_forward"
        x = _chk(x, "bottom[0]", ndim=self.axes)
        if out is not None:
            _chk(out, "top[0]", ndim=self.axes)
        (N, _, _, Cout, _, _), size = self.blobs(what, g, transposed, x, in_c0, out, out_c0)
        b = _chk_opt(bias, "bias", ndim=1)
        pw = _chk(packed, "packed weight", ndim=None)
        if pw.numel() != self.sizes(g, transposed)[0]:
            raise ValueError("%s: the operand has %d floats, not what the forward reads for this layer" % (what, pw.numel()))
        if out is None:
            out = torch.empty((N, Cout) + size, device=x.device, dtype=torch.float32)
        check(self.c("forward")(self.arg(g), int(bool(transposed)), _ptr(x), x.shape[1], int(in_c0), _ptr(pw), _ptr(b), _ptr(out), out.shape[1],
                                int(out_c0), int(bool(relu)), C.c_float(float(negative_slope)), _stream()))
        return out

    def backward_data(self, top_diff, packed, g, transposed=False, top_c0=0, out=None, out_c0=0):
        what = self.name + "_backward_data"
        d = _chk(top_diff, "top_diff", ndim=self.axes)
        if out is not None:
            _chk(out, "bottom diff", ndim=self.axes)
        (N, Cin, size, _, _, _), _ = self.blobs(what, g, transposed, out, out_c0, d, top_c0)
        pw = _chk(packed, "packed weight", ndim=None)
        if pw.numel() != self.sizes(g, transposed)[1]:
            raise ValueError("%s: the operand has %d floats, not what the data gradient reads for this layer" % (what, pw.numel()))
        if out is None:
            out = torch.empty((N, Cin) + size, device=d.device, dtype=torch.float32)
        check(self.c("backward_data")(self.arg(g), int(bool(transposed)), _ptr(d), d.shape[1], int(top_c0), _ptr(pw), _ptr(out), out.shape[1],
                                      int(out_c0), _stream()))
        return out

    def backward_weights(self, bottom, top_diff, g, transposed=False, weight_diff=None, bias_diff=None, bias=True, accumulate=False,
                         bottom_c0=0, top_c0=0):
        what = self.name + "_backward_weights"
        x, d = _chk(bottom, "bottom", ndim=self.axes), _chk(top_diff, "top_diff", ndim=self.axes)
        layer, _ = self.blobs(what, g, transposed, x, bottom_c0, d, top_c0)
        shape, Cout = self.weight_shape(layer, transposed), layer[3]
        if weight_diff is None:
            if accumulate:
                raise ValueError(what + ": accumulate needs the diffs to add into")
        elif tuple(_chk(weight_diff, "weight diff", ndim=self.axes).shape) != shape or not weight_diff.is_contiguous():
            raise ValueError(what + ": weight diff has the wrong shape")
        if bias and bias_diff is None:
            if accumulate:
                raise ValueError(what + ": accumulate needs the diffs to add into")
        elif bias and (tuple(_chk(bias_diff, "bias diff", ndim=1).shape) != (Cout,) or not bias_diff.is_contiguous()):
            raise ValueError(what + ": bias diff has the wrong shape")
        need = self.sizes(g, transposed)[3]
        if weight_diff is None:
            weight_diff = torch.empty(shape, device=x.device, dtype=torch.float32)
        if bias and bias_diff is None:
            bias_diff = torch.empty(Cout, device=x.device, dtype=torch.float32)
        ws = torch.empty((need + 3) // 4, device=x.device, dtype=torch.float32)
        check(self.c("backward_weights")(self.arg(g), int(bool(transposed)), _ptr(x), x.shape[1], int(bottom_c0), _ptr(d), d.shape[1], int(top_c0),
                                         _ptr(weight_diff), _ptr(bias_diff if bias else None), int(bool(accumulate)), _ptr(ws), need, _stream()))
        return weight_diff, (bias_diff if bias else None)


def set_conv_general_groups(groups: int = 0):
    """Test hook (fn2_debug_set_conv_general_groups): 16-channel groups per workgroup of the general gather kernels; 0 = by geometry."""
    check(_lib.lib().fn2_debug_set_conv_general_groups(int(groups)))


def conv_general_out_shape(desc, transposed=False):
    """(Hout, Wout) of the layer as the reference computes it (conv_layer.cpp:8-23, deconv_layer.cpp:8-24)."""
    k, s, p = desc.kernel, desc.stride, desc.pad
    if transposed:
        return s * (desc.Hin - 1) + k - 2 * p, s * (desc.Win - 1) + k - 2 * p
    return (desc.Hin + 2 * p - k) // s + 1, (desc.Win + 2 * p - k) // s + 1


# the square-tap ABI on fn2_conv_desc (include/flownet2_hip_conv_general.h), the 14 ints (flownet2_hip_conv_geometry.h), the 19 ints
# (flownet2_hip_conv_volume.h)
conv_general_abi = _ConvAbi("conv_general", 4, C.byref, lambda d: (d.N, d.Cin, (d.Hin, d.Win), d.Cout, (d.kernel, d.kernel), 1),
                        key=lambda d: (d.kernel, d.stride, d.pad), out_shape=conv_general_out_shape, shape_first=True)
conv_geometry_abi = _ConvAbi("conv_geometry", 4, lambda g: g, lambda g: (g[0], g[1], (g[2], g[3]), g[4], (g[5], g[6]), g[13]))
conv_volume_abi = _ConvAbi("conv_volume", 5, lambda g: g, lambda g: (g[0], g[1], tuple(g[2:5]), g[5], tuple(g[6:9]), g[18]), sep=", ")


def conv_general_supported(desc, transposed=False) -> bool:
    """Whether the general-geometry kernels (csrc/conv_general.hip) take this layer (fn2_conv_general_supported; host-only)."""
    return conv_general_abi.supported(desc, transposed)


def conv_general_sizes(desc, transposed=False):
    """(floats of the forward operand, of the data-gradient operand, of the weight-gradient operand (0), bytes of the weight-gradient
    workspace) of the general kernels (fn2_conv_general_sizes; host-only)."""
    return conv_general_abi.sizes(desc, transposed)


def conv_general_pack_weights(weight, desc, transposed=False, backward=False):
    """The layer's weight blob -> the operand of the general forward (backward: data-gradient) kernel (fn2_conv_general_pack_weights)."""
    return conv_general_abi.pack_weights(weight, desc, transposed, backward)


def conv_general_forward(x, packed, bias, desc, transposed=False, relu=False, negative_slope=0.0, out=None, out_c0=0, in_c0=0):
    """act(layer(x[:, in_c0:in_c0+Cin]) + bias) -> out[:, out_c0:out_c0+Cout] (a new blob if out is None) on the general kernel
    (fn2_conv_general_forward).  packed = conv_general_pack_weights(weight, desc, transposed)."""
    return conv_general_abi.forward(x, packed, bias, desc, transposed, relu, negative_slope, out, out_c0, in_c0)


def conv_general_backward_data(top_diff, packed, desc, transposed=False, top_c0=0, out=None, out_c0=0):
    """bottom_diff [N, Cin, Hin, Win] (or the slice of `out` at out_c0) of the layer on the general kernel (fn2_conv_general_backward_data).
    packed = conv_general_pack_weights(weight, desc, transposed, backward=True)."""
    return conv_general_abi.backward_data(top_diff, packed, desc, transposed, top_c0, out, out_c0)


def conv_general_backward_weights(bottom, top_diff, desc, transposed=False, weight_diff=None, bias_diff=None, bias=True, accumulate=False,
                                  bottom_c0=0, top_c0=0):
    """(weight_diff, bias_diff) of the layer on the general kernels (fn2_conv_general_backward_weights; deterministic).  accumulate adds
    into the diffs given; bias=False: no bias gradient (None comes back)."""
    return conv_general_abi.backward_weights(bottom, top_diff, desc, transposed, weight_diff, bias_diff, bias, accumulate, bottom_c0, top_c0)


def _pair(v, what):
    """An int or a pair -> (h, w)."""
    if isinstance(v, (tuple, list)):
        if len(v) == 1:
            return int(v[0]), int(v[0])
        if len(v) != 2:
            raise ValueError(f"{what}: one value or a pair, not {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def conv_geometry(N, Cin, Hin, Win, Cout, kernel, stride=1, pad=0, dilation=1, group=1):
    """The 14 ints of include/flownet2_hip_conv_geometry.h: {N, Cin, Hin, Win, Cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
    dilation_h, dilation_w, group}; kernel, stride, pad and dilation an int or a pair (h, w)."""
    vals = (N, Cin, Hin, Win, Cout) + _pair(kernel, "kernel") + _pair(stride, "stride") + _pair(pad, "pad") + _pair(dilation, "dilation") + (group,)
    return (C.c_int * 14)(*(int(v) for v in vals))


def conv_geometry_supported(geom, transposed=False) -> bool:
    """Whether the general-geometry kernels take this layer (fn2_conv_geometry_supported; host-only)."""
    return conv_geometry_abi.supported(geom, transposed)


def conv_geometry_sizes(geom, transposed=False):
    """(floats of the forward operand, of the data-gradient operand, of the weight-gradient operand (0), bytes of the weight-gradient
    workspace) (fn2_conv_geometry_sizes; host-only)."""
    return conv_geometry_abi.sizes(geom, transposed)


def conv_geometry_out_shape(geom, transposed=False):
    """(Hout, Wout) of the layer as the reference computes it with the dilated extent (fn2_conv_geometry_out_shape; host-only)."""
    return conv_geometry_abi.c_out_shape(geom, transposed)


def conv_geometry_pack_weights(weight, geom, transposed=False, backward=False):
    """The layer's weight blob -> the operand of the forward (backward: data-gradient) kernel (fn2_conv_geometry_pack_weights)."""
    return conv_geometry_abi.pack_weights(weight, geom, transposed, backward)


def conv_geometry_forward(x, packed, bias, geom, transposed=False, relu=False, negative_slope=0.0, out=None, out_c0=0, in_c0=0):
    """act(layer(x[:, in_c0:in_c0+Cin]) + bias) -> out[:, out_c0:out_c0+Cout] (a new blob if out is None) (fn2_conv_geometry_forward).
    packed = conv_geometry_pack_weights(weight, geom, transposed)."""
    return conv_geometry_abi.forward(x, packed, bias, geom, transposed, relu, negative_slope, out, out_c0, in_c0)


def conv_geometry_backward_data(top_diff, packed, geom, transposed=False, top_c0=0, out=None, out_c0=0):
    """bottom_diff [N, Cin, Hin, Win] (or the slice of `out` at out_c0) of the layer (fn2_conv_geometry_backward_data).
    packed = conv_geometry_pack_weights(weight, geom, transposed, backward=True)."""
    return conv_geometry_abi.backward_data(top_diff, packed, geom, transposed, top_c0, out, out_c0)


def conv_geometry_backward_weights(bottom, top_diff, geom, transposed=False, weight_diff=None, bias_diff=None, bias=True, accumulate=False,
                                   bottom_c0=0, top_c0=0):
    """(weight_diff, bias_diff) of the layer (fn2_conv_geometry_backward_weights; deterministic).  accumulate adds into the diffs given;
    bias=False: no bias gradient (None comes back)."""
    return conv_geometry_abi.backward_weights(bottom, top_diff, geom, transposed, weight_diff, bias_diff, bias, accumulate, bottom_c0, top_c0)


def _per_axis(v, axes, what):
    """An int or one value per spatial axis -> `axes` ints."""
    if isinstance(v, (tuple, list)):
        if len(v) == 1:
            return (int(v[0]),) * axes
        if len(v) != axes:
            raise ValueError(f"{what}: one value or one per spatial axis ({axes}), not {v!r}")
        return tuple(int(s) for s in v)
    return (int(v),) * axes


def conv_volume(N, Cin, size, Cout, kernel, stride=1, pad=0, dilation=1, group=1):
    """The 19 ints of include/flownet2_hip_conv_volume.h: {N, Cin, Din, Hin, Win, Cout, kernel_d/h/w, stride_d/h/w, pad_d/h/w,
    dilation_d/h/w, group}.  size: the 0 to 3 spatial extents of the bottom blob, outermost first; kernel, stride, pad and dilation an int
    or one value per spatial axis.  Fewer than three axes are folded onto the innermost ones (the leading axes trivial: extent 1, kernel 1,
    stride 1, pad 0, dilation 1); N is the folded batch."""
    size = tuple(int(s) for s in size)
    axes = len(size)
    if axes > 3:
        raise ValueError(f"conv_volume: {axes} spatial axes asked for; convolution over 0 to 3 spatial axes is supported")
    lead = 3 - axes
    vals = ((N, Cin) + (1,) * lead + size + (Cout,) + (1,) * lead + _per_axis(kernel, axes, "kernel") + (1,) * lead + _per_axis(stride, axes, "stride")
            + (0,) * lead + _per_axis(pad, axes, "pad") + (1,) * lead + _per_axis(dilation, axes, "dilation") + (group,))
    return (C.c_int * 19)(*(int(v) for v in vals))


def conv_volume_supported(geom, transposed=False) -> bool:
    """Whether the general kernels take this layer (fn2_conv_volume_supported; host-only)."""
    return conv_volume_abi.supported(geom, transposed)


def conv_volume_sizes(geom, transposed=False):
    """(floats of the forward operand, of the data-gradient operand, of the weight-gradient operand (0), bytes of the weight-gradient
    workspace) (fn2_conv_volume_sizes; host-only)."""
    return conv_volume_abi.sizes(geom, transposed)


def conv_volume_out_shape(geom, transposed=False):
    """(Dout, Hout, Wout) of the layer as the reference computes it with the dilated extent (fn2_conv_volume_out_shape; host-only)."""
    return conv_volume_abi.c_out_shape(geom, transposed)


def conv_volume_pack_weights(weight, geom, transposed=False, backward=False):
    """The layer's weight blob [., ., kd, kh, kw] -> the operand of the forward (backward: data-gradient) kernel (fn2_conv_volume_pack_weights)."""
    return conv_volume_abi.pack_weights(weight, geom, transposed, backward)


def conv_volume_forward(x, packed, bias, geom, transposed=False, relu=False, negative_slope=0.0, out=None, out_c0=0, in_c0=0):
    """act(layer(x[:, in_c0:in_c0+Cin]) + bias) -> out[:, out_c0:out_c0+Cout] (a new blob if out is None) on [N, C, D, H, W] blobs
    (fn2_conv_volume_forward).  packed = conv_volume_pack_weights(weight, geom, transposed)."""
    return conv_volume_abi.forward(x, packed, bias, geom, transposed, relu, negative_slope, out, out_c0, in_c0)


def conv_volume_backward_data(top_diff, packed, geom, transposed=False, top_c0=0, out=None, out_c0=0):
    """bottom_diff [N, Cin, Din, Hin, Win] (or the slice of `out` at out_c0) of the layer (fn2_conv_volume_backward_data).
    packed = conv_volume_pack_weights(weight, geom, transposed, backward=True)."""
    return conv_volume_abi.backward_data(top_diff, packed, geom, transposed, top_c0, out, out_c0)


def conv_volume_backward_weights(bottom, top_diff, geom, transposed=False, weight_diff=None, bias_diff=None, bias=True, accumulate=False,
                                 bottom_c0=0, top_c0=0):
    """(weight_diff, bias_diff) of the layer (fn2_conv_volume_backward_weights; deterministic).  accumulate adds into the diffs given;
    bias=False: no bias gradient (None comes back)."""
    return conv_volume_abi.backward_weights(bottom, top_diff, geom, transposed, weight_diff, bias_diff, bias, accumulate, bottom_c0, top_c0)


def conv_mfma_supported(Cin, Hin, Win, Cout, kernel, stride, pad) -> bool:
    return bool(_lib.lib().fn2_conv_mfma_supported(int(Cin), int(Hin), int(Win), int(Cout), int(kernel), int(stride), int(pad)))


def conv_mfma_pack_weights(weight):
    """weight [Cout, Cin, k, k] -> the MFMA operand order fn2_conv_mfma_forward reads (once per weight update)."""
    w = _chk(weight, "weight")
    Cout, Cin, k, k2 = w.shape
    n = _lib.lib().fn2_conv_mfma_packed_floats(Cout, Cin, k)
    if k != k2 or n == 0:
        raise ValueError(f"conv_mfma: unsupported weight shape {tuple(w.shape)}")
    return _packed(w, n, _lib.lib().fn2_conv_mfma_pack_weights, Cout, Cin, k)


def conv_mfma_pack_weights_view(blob, Cout, Cin, kernel, src_cout, src_cin, stride_cout, stride_cin, flip=False):
    """The operand fn2_conv_mfma_forward reads for the strided [Cout][Cin][k][k] VIEW of a contiguous weight blob: element (co, ci, tap) =
    blob.flatten()[co * stride_cout + ci * stride_cin + (k*k - 1 - tap if flip else tap)] for co < src_cout, ci < src_cin, 0 beyond --
    channel-swapped, rotated and zero-padded operands in one launch (csrc/conv_mfma.hip: pack_weights_view)."""
    w = _chk(blob, "weight", ndim=blob.dim())
    if not w.is_contiguous():
        raise ValueError("conv_mfma_pack_weights_view: the blob itself must be contiguous (the view is described by the strides)")
    n = _lib.lib().fn2_conv_mfma_packed_floats(int(Cout), int(Cin), int(kernel))
    if n == 0:
        raise ValueError(f"conv_mfma: unsupported operand [{Cout},{Cin},{kernel},{kernel}]")
    last = (src_cout - 1) * stride_cout + (src_cin - 1) * stride_cin + kernel * kernel - 1
    if last >= w.numel():
        raise ValueError("conv_mfma_pack_weights_view: the view reaches beyond the blob")
    return _packed(w, n, _lib.lib().fn2_conv_mfma_pack_weights_view, int(Cout), int(Cin), int(kernel), int(src_cout), int(src_cin),
                   int(stride_cout), int(stride_cin), int(bool(flip)))


def conv_mfma_forward(x, packed_weight, bias, Cout, kernel, stride, pad, relu=True, negative_slope=0.1, out=None, out_c0=0,
                      in_c0=0, Cin=None):
    """act(Convolution{kernel, stride, pad}(x[:, in_c0:in_c0+Cin]) + bias) -> out[:, out_c0:out_c0+Cout] (a new blob if out is None)."""
    x = _chk(x, "bottom[0]")
    N, Ctot, H, W = x.shape
    Cin = Ctot - in_c0 if Cin is None else Cin
    out = _top("conv_mfma", out, N, Cout, (H + 2 * pad - kernel) // stride + 1, (W + 2 * pad - kernel) // stride + 1, x.device)
    b, pw = _chk_opt(bias, "bias", 1), _chk(packed_weight, "packed weight", ndim=1)
    check(_lib.lib().fn2_conv_mfma_forward(_ptr(x), _ptr(pw), _ptr(b), _ptr(out), N, Cin, H, W, Ctot, in_c0, Cout, out.shape[1], out_c0,
                                           kernel, stride, pad, int(bool(relu)), C.c_float(float(negative_slope)), _stream()))
    return out


def set_conv_variant(v: int):
    check(_lib.lib().fn2_debug_set_conv_variant(int(v)))


def conv_num_variants() -> int:
    return int(_lib.lib().fn2_conv_mfma_num_variants())


def conv_wino_supported(Cin, Hin, Win, Cout, pad) -> bool:
    return bool(_lib.lib().fn2_conv_wino_supported(int(Cin), int(Hin), int(Win), int(Cout), int(pad)))


def conv_wino_pack_weights(weight):
    """weight [Cout, Cin, 3, 3] -> U = G g G^T in MFMA operand order (once per weight update)."""
    w = _chk(weight, "weight")
    Cout, Cin, k, k2 = w.shape
    n = _lib.lib().fn2_conv_wino_packed_floats(Cout, Cin)
    if k != 3 or k2 != 3 or n == 0:
        raise ValueError(f"conv_wino: unsupported weight shape {tuple(w.shape)}")
    return _packed(w, n, _lib.lib().fn2_conv_wino_pack_weights, Cout, Cin)


def conv_wino_forward(x, packed_weight, bias, Cout, pad=1, relu=True, negative_slope=0.1, out=None, out_c0=0, in_c0=0, Cin=None):
    """act(Convolution{3, 1, pad}(x[:, in_c0:in_c0+Cin]) + bias) -> out[:, out_c0:out_c0+Cout], Winograd F(2x2, 3x3)."""
    x = _chk(x, "bottom[0]")
    N, Ctot, H, W = x.shape
    Cin = Ctot - in_c0 if Cin is None else Cin
    out = _top("conv_wino", out, N, Cout, H + 2 * pad - 2, W + 2 * pad - 2, x.device)
    b, pw = _chk_opt(bias, "bias", 1), _chk(packed_weight, "packed weight", ndim=1)
    check(_lib.lib().fn2_conv_wino_forward(_ptr(x), _ptr(pw), _ptr(b), _ptr(out), N, Cin, H, W, Ctot, in_c0, Cout, out.shape[1], out_c0,
                                           pad, int(bool(relu)), C.c_float(float(negative_slope)), _stream()))
    return out


def conv_plane_supported(N, Cin, Hin, Win, Cout, stride, pad) -> bool:
    return bool(_lib.lib().fn2_conv_plane_supported(int(N), int(Cin), int(Hin), int(Win), int(Cout), int(stride), int(pad)))


def conv_plane_ksplit(N, Cin, Hin, Win, Cout, stride, pad) -> int:
    return int(_lib.lib().fn2_conv_plane_ksplit(int(N), int(Cin), int(Hin), int(Win), int(Cout), int(stride), int(pad)))


_PLANE_WS = {}      # (device, stream) -> the split-K partial-sum workspace (grown on demand, reused by every layer: launches are stream-ordered)
_PLANE_WS_RETIRED = []   # outgrown workspaces are kept alive: a hipGraph captured earlier has their address baked into its kernels


def _plane_workspace(device, need):
    """Per (device, stream) scratch of at least `need` bytes.  Never freed or shrunk: a regrow keeps the old block alive
    (_PLANE_WS_RETIRED), so a graph captured with the old pointer keeps replaying into memory nobody else owns; separate streams get
    separate blocks (no ordering exists between them)."""
    key = (device, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _PLANE_WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        if ws is not None:
            _PLANE_WS_RETIRED.append(ws)
        ws = _PLANE_WS[key] = torch.empty((need + 3) // 4, device=device, dtype=torch.float32)
    return ws


def _scratch(device, need):
    """What a *_workspace_bytes() query answered -> (that much of the per-stream scratch, or None for 0; the bytes as an int)."""
    need = int(need)
    return (_plane_workspace(device, need) if need else None), need


def conv_plane_k_supported(N, Cin, Hin, Win, Cout, kernel, stride, pad) -> bool:
    return bool(_lib.lib().fn2_conv_plane_k_supported(int(N), int(Cin), int(Hin), int(Win), int(Cout), int(kernel), int(stride), int(pad)))


def conv_plane_k_ksplit(N, Cin, Hin, Win, Cout, kernel, stride, pad) -> int:
    return int(_lib.lib().fn2_conv_plane_k_ksplit(int(N), int(Cin), int(Hin), int(Win), int(Cout), int(kernel), int(stride), int(pad)))


def conv_plane_forward(x, packed_weight, bias, Cout, stride, pad, relu=True, negative_slope=0.1, out=None, out_c0=0, in_c0=0, Cin=None, kernel=3):
    """act(Convolution{kernel, stride, pad}(x[:, in_c0:in_c0+Cin]) + bias) -> out[:, out_c0:out_c0+Cout] for small feature maps
    (csrc/conv_plane.hip); kernel 3, 4 with stride 2 / pad 1, or 5 with stride 2 / pad 2; packed_weight = conv_mfma_pack_weights(weight)."""
    x = _chk(x, "bottom[0]")
    N, Ctot, H, W = x.shape
    Cin = Ctot - in_c0 if Cin is None else Cin
    out = _top("conv_plane", out, N, Cout, (H + 2 * pad - kernel) // stride + 1, (W + 2 * pad - kernel) // stride + 1, x.device)
    b, pw = _chk_opt(bias, "bias", 1), _chk(packed_weight, "packed weight", ndim=1)
    ws, need = _scratch(x.device, _lib.lib().fn2_conv_plane_k_workspace_bytes(N, Cin, H, W, Cout, kernel, stride, pad))
    check(_lib.lib().fn2_conv_plane_k_forward(_ptr(x), _ptr(pw), _ptr(b), _ptr(out), N, Cin, H, W, Ctot, in_c0, Cout, out.shape[1], out_c0,
                                              kernel, stride, pad, int(bool(relu)), C.c_float(float(negative_slope)), _ptr(ws), need, _stream()))
    return out


def tconv_supported(Cin, Hin, Win, Cout, Hout, Wout, kernel, pad) -> bool:
    return bool(_lib.lib().fn2_tconv_supported(int(Cin), int(Hin), int(Win), int(Cout), int(Hout), int(Wout), int(kernel), int(pad)))


def tconv_pack_weights(weight):
    """weight [Cin, Cout, k, k] (Caffe's Deconvolution blob; for a data gradient the Convolution's own [Cout_conv, Cin_conv, k, k] blob)
    -> the MFMA operand order fn2_tconv_forward reads: fn2_conv_mfma_pack_weights of the [Cout][Cin][k][k] view."""
    w = weight.detach().contiguous()
    A, B, k, _ = w.shape                                    # operand [Cout = B][Cin = A][k][k]: the blob with its channel axes swapped
    return conv_mfma_pack_weights_view(w, B, A, k, B, A, k * k, B * k * k)


def tconv_forward(x, packed_weight, bias, Cout, kernel, pad, out_hw=None, relu=False, negative_slope=0.1, out=None, out_c0=0, in_c0=0, Cin=None):
    """Transposed convolution, stride 2 (csrc/tconv_mfma.hip): the Deconvolution forward (+ bias + ReLU) or a stride-2 Convolution's
    data gradient.  out_hw: output size (default 2 (H - 1) + kernel - 2 pad)."""
    x = _chk(x, "bottom[0]")
    N, Ctot, H, W = x.shape
    Cin = Ctot - in_c0 if Cin is None else Cin
    Ho, Wo = out_hw if out_hw is not None else (2 * (H - 1) + kernel - 2 * pad, 2 * (W - 1) + kernel - 2 * pad)
    out = _top("tconv", out, N, Cout, Ho, Wo, x.device)
    b, pw = _chk_opt(bias, "bias", 1), _chk(packed_weight, "packed weight", ndim=1)
    check(_lib.lib().fn2_tconv_forward(_ptr(x), _ptr(pw), _ptr(b), _ptr(out), N, Cin, H, W, Ctot, in_c0, Cout, Ho, Wo, out.shape[1], out_c0,
                                       int(kernel), int(pad), int(bool(relu)), C.c_float(float(negative_slope)), _stream()))
    return out


def set_tconv_variant(v: int):
    check(_lib.lib().fn2_debug_set_tconv_variant(int(v)))


def tconv_num_variants() -> int:
    return int(_lib.lib().fn2_tconv_num_variants())


def conv_wgrad_supported(N, Ca, Ha, Wa, Cb, Hb, Wb, kernel, stride, pad) -> bool:
    return bool(_lib.lib().fn2_conv_wgrad_supported(int(N), int(Ca), int(Ha), int(Wa), int(Cb), int(Hb), int(Wb), int(kernel), int(stride), int(pad)))


def conv_wgrad_ksplit(N, Ca, Ha, Wa, Cb, Hb, Wb, kernel, stride, pad) -> int:
    return int(_lib.lib().fn2_conv_wgrad_ksplit(int(N), int(Ca), int(Ha), int(Wa), int(Cb), int(Hb), int(Wb), int(kernel), int(stride), int(pad)))


def conv_wgrad(a, b, kernel, stride, pad, out=None, accumulate=False, a_c0=0, Ca=None, b_c0=0, Cb=None):
    """dw[ca][cb][ky][kx] (+)= sum a[n, a_c0 + ca, y, x] * b[n, b_c0 + cb, stride y + ky - pad, stride x + kx - pad] (csrc/conv_wgrad.hip).
    Convolution: a = top_diff, b = bottom -> [Cout, Cin, k, k]; Deconvolution: a = bottom, b = top_diff -> [Cin, Cout, k, k]."""
    a, b = _chk(a, "a"), _chk(b, "b")
    N, Atot, Ha, Wa = a.shape
    Nb, Btot, Hb, Wb = b.shape
    if N != Nb:
        raise ValueError("conv_wgrad: batch sizes differ")
    Ca = Atot - a_c0 if Ca is None else Ca
    Cb = Btot - b_c0 if Cb is None else Cb
    if out is None:
        out = torch.empty((Ca, Cb, kernel, kernel), device=a.device, dtype=torch.float32)
        accumulate = False
    else:
        out = _chk(out, "weight diff")
        if tuple(out.shape) != (Ca, Cb, kernel, kernel):
            raise ValueError("conv_wgrad: weight diff has the wrong shape")
    ws, need = _scratch(a.device, _lib.lib().fn2_conv_wgrad_workspace_bytes(N, Ca, Ha, Wa, Cb, Hb, Wb, kernel, stride, pad))
    check(_lib.lib().fn2_conv_wgrad(_ptr(a), _ptr(b), _ptr(out), N, Ca, Ha, Wa, Atot, a_c0, Cb, Hb, Wb, Btot, b_c0, int(kernel), int(stride), int(pad),
                                    int(bool(accumulate)), _ptr(ws), need, _stream()))
    return out


def deconv_plane_supported(N, Cin, Hin, Win, Cout) -> bool:
    return bool(_lib.lib().fn2_deconv_plane_supported(int(N), int(Cin), int(Hin), int(Win), int(Cout)))


def deconv_plane_ksplit(N, Cin, Hin, Win, Cout) -> int:
    return int(_lib.lib().fn2_deconv_plane_ksplit(int(N), int(Cin), int(Hin), int(Win), int(Cout)))


def deconv_plane_pack_weights(weight):
    """weight [Cin, Cout, 4, 4] (Caffe's deconvolution blob) -> per-parity-class MFMA operand order (once per weight update).  A
    [Cin, Cout, 3, 3] blob is read as the 4x4 one whose fourth tap row and column are zero (the transposed 3x3 / 2 / 1 convolution of a
    data gradient on a small map), without a padded copy."""
    w = _chk(weight, "weight")
    Cin, Cout, k, k2 = w.shape
    n = _lib.lib().fn2_deconv_plane_packed_floats(Cin, Cout)
    if k not in (3, 4) or k2 != k or n == 0:
        raise ValueError(f"deconv_plane: unsupported weight shape {tuple(w.shape)}")
    return _packed(w, n, _lib.lib().fn2_deconv_plane_pack_weights_k, Cin, Cout, k)


def deconv_plane_forward(x, packed_weight, bias, Cout, relu=True, negative_slope=0.1, out=None, out_c0=0, in_c0=0, Cin=None):
    """act(Deconvolution{4, 2, 1}(x[:, in_c0:in_c0+Cin]) + bias) -> out[:, out_c0:out_c0+Cout] (csrc/conv_plane.hip, MODE 1)."""
    x = _chk(x, "bottom[0]")
    N, Ctot, H, W = x.shape
    Cin = Ctot - in_c0 if Cin is None else Cin
    out = _top("deconv_plane", out, N, Cout, 2 * H, 2 * W, x.device)
    b, pw = _chk_opt(bias, "bias", 1), _chk(packed_weight, "packed weight", ndim=1)
    ws, need = _scratch(x.device, _lib.lib().fn2_deconv_plane_workspace_bytes(N, Cin, H, W, Cout))
    check(_lib.lib().fn2_deconv_plane_forward(_ptr(x), _ptr(pw), _ptr(b), _ptr(out), N, Cin, H, W, Ctot, in_c0, Cout, out.shape[1], out_c0,
                                              int(bool(relu)), C.c_float(float(negative_slope)), _ptr(ws), need, _stream()))
    return out


def set_plane_variant(v: int):
    check(_lib.lib().fn2_debug_set_plane_variant(int(v)))


def set_plane_ksplit(k: int):
    check(_lib.lib().fn2_debug_set_plane_ksplit(int(k)))


def set_batch_invariant(on: bool):
    """fn2_set_batch_invariant: summation orders that would depend on N are computed for a batch of one sample."""
    check(_lib.lib().fn2_set_batch_invariant(1 if on else 0))


def get_batch_invariant() -> bool:
    return bool(_lib.lib().fn2_get_batch_invariant())


def plane_num_variants() -> int:
    return int(_lib.lib().fn2_conv_plane_num_variants())


def set_wino_variant(v: int):
    check(_lib.lib().fn2_debug_set_wino_variant(int(v)))


def wino_num_variants() -> int:
    return int(_lib.lib().fn2_conv_wino_num_variants())


def im2col_forward(x, kernel, pad, stride):
    """[N,C,H,W] -> col [N, C*k*k, Hc*Wc] (Caffe's im2col row order), batched."""
    x = _chk(x, "bottom[0]")
    N, Cc, H, W = x.shape
    Hc, Wc = (H + 2 * pad - kernel) // stride + 1, (W + 2 * pad - kernel) // stride + 1
    col = torch.empty((N, Cc * kernel * kernel, Hc * Wc), device=x.device, dtype=torch.float32)
    check(_lib.lib().fn2_im2col_forward(_ptr(x), _ptr(col), N, Cc, H, W, int(kernel), int(pad), int(stride), _stream()))
    return col


def col2im_bias_relu_forward(col, bias, N, Cc, H, W, kernel, pad, stride, relu=True, negative_slope=0.1, out=None, out_c0=0):
    """col [N, C*k*k, Hc*Wc] -> image [N,C,H,W] (+ bias[c], optional leaky ReLU): the tail of a Deconvolution forward; with `out` the
    image goes to out[:, out_c0:out_c0+C] of a wider blob."""
    if not (col.is_cuda and col.dtype == torch.float32 and col.is_contiguous()):
        raise ValueError("col2im: expected a contiguous float32 CUDA (HIP) column blob")
    Hc, Wc = (H + 2 * pad - kernel) // stride + 1, (W + 2 * pad - kernel) // stride + 1
    if col.numel() != N * Cc * kernel * kernel * Hc * Wc:
        raise ValueError(f"col2im: column blob has {col.numel()} entries, expected {N * Cc * kernel * kernel * Hc * Wc}")
    b = _chk_opt(bias, "bias", 1)
    if out is not None:
        _top("col2im", out, N, Cc, H, W, col.device)
        check(_lib.lib().fn2_col2im_bias_relu_forward_into(_ptr(col), _ptr(b), _ptr(out), N, Cc, H, W, int(kernel), int(pad), int(stride),
                                                           int(bool(relu)), C.c_float(float(negative_slope)), out.shape[1], int(out_c0), _stream()))
        return out[:, out_c0:out_c0 + Cc]
    out = torch.empty((N, Cc, H, W), device=col.device, dtype=torch.float32)
    check(_lib.lib().fn2_col2im_bias_relu_forward(_ptr(col), _ptr(b), _ptr(out), N, Cc, H, W, int(kernel), int(pad), int(stride),
                                                  int(bool(relu)), C.c_float(float(negative_slope)), _stream()))
    return out


def bias_leaky_relu_backward(top_data, top_diff, negative_slope=0.1, need_bias_diff=True):
    """(bottom_diff, bias_diff): gradient of x -> leaky_relu(x + bias) given the OUTPUT blob and its gradient.  Either may be a channel slice
    (blob, c0, C) of a wider blob -- the gradient a Concat hands its bottoms; an output that was written straight into its consumer's Concat
    blob -- and is then read in place."""
    y, yctot, yc0, Cc = _as_slice(top_data, "top.data")
    g, gctot, gc0, gC = _as_slice(top_diff, "top.diff")
    N, _, H, W = y.shape
    if gC != Cc or g.shape[0] != N or tuple(g.shape[2:]) != (H, W):
        raise ValueError("top.data and top.diff must have the same shape")
    d = torch.empty((N, Cc, H, W), device=y.device, dtype=torch.float32)
    db = torch.empty(Cc, device=y.device, dtype=torch.float32) if need_bias_diff else None
    nbytes = _lib.lib().fn2_bias_leaky_relu_backward_workspace_bytes(N, Cc, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=y.device)
    check(_lib.lib().fn2_bias_leaky_relu_backward_slices2(_ptr(y), yctot, yc0, _ptr(g), gctot, gc0, _ptr(d), _ptr(db), N, Cc, H, W,
                                                          C.c_float(float(negative_slope)), _ptr(ws), nbytes, _stream()))
    return d, db


AUG_NUM_PARAMS, = _consts("AUG_NUM_PARAMS")      # AugmentationCoeff fields, caffe.proto:436-486


def augmentation_matrix(coeffs, crop_width, crop_height, bottom_width, bottom_height, invert=False):
    """HOST: one coefficient array (coeff_to_array layout) -> (t0, t1, t2, t3, t4, t5) of tTransMat::fromCoeff (optionally inverted)."""
    import numpy as np
    c = np.ascontiguousarray(coeffs, np.float32)
    if c.shape != (AUG_NUM_PARAMS,):
        raise ValueError(f"coefficient array must have {AUG_NUM_PARAMS} entries")
    out = np.empty(6, np.float32)
    check(_lib.lib().fn2_augmentation_matrix(C.c_void_p(c.ctypes.data), crop_width, crop_height, bottom_width, bottom_height, int(invert),
                                             C.c_void_p(out.ctypes.data)))
    return out


def flow_augmentation_forward(flow, coeffs1, coeffs2, crop_height, crop_width):
    """flow: CUDA [N,2,H,W]; coeffs1 / coeffs2: [N,42] coefficient arrays of image 1 / image 2 (read on the host, like the reference's
    cpu_data(), flow_augmentation_layer.cu:123-124).  Returns [N,2,crop_height,crop_width]."""
    import numpy as np
    fl = _chk(flow, "bottom[0] (flow)")
    N, Cc, H, W = fl.shape
    if Cc != 2:
        raise ValueError("Flow data must have two channels")                      # flow_augmentation_layer.cpp:52
    host = []
    for c in (coeffs1, coeffs2):
        a = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
        a = np.ascontiguousarray(a, np.float32).reshape(N, -1)
        if a.shape[1] != AUG_NUM_PARAMS:
            raise ValueError(f"coefficient blobs must hold {AUG_NUM_PARAMS} values per sample")
        host.append(a)
    top = torch.empty((N, 2, int(crop_height), int(crop_width)), device=fl.device, dtype=torch.float32)
    check(_lib.lib().fn2_flow_augmentation_forward(_ptr(fl), C.c_void_p(host[0].ctypes.data), C.c_void_p(host[1].ctypes.data), _ptr(top),
                                                   N, H, W, int(crop_height), int(crop_width), _stream()))
    return top


MEAN_NONE, MEAN_PER_CHANNEL, MEAN_PER_PIXEL = _consts("MEAN_NONE", "MEAN_PER_CHANNEL", "MEAN_PER_PIXEL")


def data_aug_params(crop_width=0, crop_height=0, max_multiplier=255.0, chromatic_eigvec=None, mean_mode=MEAN_NONE, noise_seed=0, noise_stream=0):
    p = _lib.DataAugParams(int(crop_width), int(crop_height), float(max_multiplier), int(chromatic_eigvec is not None))
    p.noise_seed, p.noise_stream = int(noise_seed), int(noise_stream)
    if chromatic_eigvec is not None:
        if len(chromatic_eigvec) != 9:
            raise ValueError("chromatic_eigvec must have 9 entries")
        p.chromatic_eigvec = (C.c_float * 9)(*[float(v) for v in chromatic_eigvec])
    p.mean_mode = int(mean_mode)
    return p


def data_augmentation_forward(p, bottom, coeffs=None, mean=None):
    """bottom: CUDA [N,C,H,W]; coeffs: [N,42] coefficient arrays (host side, like the reference's cpu_data()) or None = defaults;
    mean: CUDA tensor of C (per channel) or C*crop_h*crop_w (per pixel) values, as p.mean_mode says.  Returns [N,C,crop_h,crop_w]."""
    import numpy as np
    x = _chk(bottom, "bottom[0]")
    N, Cc, H, W = x.shape
    crop = p.crop_width > 0 and p.crop_height > 0
    ch, cw = (p.crop_height, p.crop_width) if crop else (H, W)
    host = None
    if coeffs is not None:
        host = coeffs.detach().cpu().numpy() if isinstance(coeffs, torch.Tensor) else np.asarray(coeffs)
        host = np.ascontiguousarray(host, np.float32).reshape(N, -1)
        if host.shape[1] != AUG_NUM_PARAMS:
            raise ValueError(f"coefficient blob must hold {AUG_NUM_PARAMS} values per sample")
    m = None
    if p.mean_mode != MEAN_NONE:
        m = _chk(mean, "mean", ndim=None)
        want = Cc if p.mean_mode == MEAN_PER_CHANNEL else Cc * ch * cw
        if m.numel() != want:
            raise ValueError(f"mean: expected {want} values")
    top = torch.empty((N, Cc, max(ch, 0), max(cw, 0)), device=x.device, dtype=torch.float32)
    nws = _lib.lib().fn2_data_augmentation_workspace_bytes(N)
    ws = torch.empty(nws, device=x.device, dtype=torch.uint8)
    check(_lib.lib().fn2_data_augmentation_forward(C.byref(p), _ptr(x), C.c_void_p(host.ctypes.data) if host is not None else None, _ptr(m),
                                                   _ptr(top), N, Cc, H, W, _ptr(ws), nws, _stream()))
    return top


# ---- solver update (include/flownet2_hip_solver.h, csrc/solver_update.hip) ------------------------------------------------------------
SOLVER_SGD, SOLVER_ADAM = _consts("SOLVER_SGD", "SOLVER_ADAM")
SOLVER_REG_L2, SOLVER_REG_L1 = _consts("SOLVER_REG_L2", "SOLVER_REG_L1")
SOLVER_CHUNK, = _consts("SOLVER_CHUNK")   # elements per chunk-list entry (one workgroup each)


def solver_params(type=SOLVER_SGD, regularization=SOLVER_REG_L2, momentum=0.0, momentum2=0.999, delta=1e-8, weight_decay=0.0,
                  clip_gradients=-1.0, accum_normalization=1.0) -> "_lib.SolverParams":
    return _lib.SolverParams(int(type), int(regularization), float(momentum), float(momentum2), float(delta), float(weight_decay),
                             float(clip_gradients), float(accum_normalization))


def _solver_tensor(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA (HIP) tensor; flownet2_amd has no CPU path")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 tensor, got {t.dtype}, strides {t.stride()}")
    return t


class SolverTable:
    """The device-resident descriptor table of one set of blobs (fn2_solver_table_build): {data, diff, hist0, hist1, count, lr_mult,
    decay_mult} per blob, the chunk list and the clip partials, plus the host-side fn2_solver_table_info.  Holds the tensors it points
    to; `ptrs` are their addresses at build time (`matches()` compares them with the tensors a caller holds now)."""

    def __init__(self, data, diff, hist0, hist1=None, lr_mults=None, decay_mults=None):
        n = len(data)
        hist1 = list(hist1) if hist1 is not None else [None] * n
        if not (len(diff) == len(hist0) == len(hist1) == n):
            raise ValueError("solver table: data, diff, hist0 and hist1 must list the same number of blobs")
        lr_mults = [1.0] * n if lr_mults is None else [float(v) for v in lr_mults]
        decay_mults = [1.0] * n if decay_mults is None else [float(v) for v in decay_mults]
        if len(lr_mults) != n or len(decay_mults) != n:
            raise ValueError("solver table: one lr_mult and one decay_mult per blob")
        blobs = (_lib.SolverBlob * max(1, n))()
        for k in range(n):
            w, g, h0 = _solver_tensor(data[k], f"data[{k}]"), _solver_tensor(diff[k], f"diff[{k}]"), _solver_tensor(hist0[k], f"hist0[{k}]")
            h1 = _solver_tensor(hist1[k], f"hist1[{k}]") if hist1[k] is not None else None
            for t, name in ((g, "diff"), (h0, "hist0"), (h1, "hist1")):
                if t is not None and (t.numel() != w.numel() or t.device != w.device):
                    raise ValueError(f"{name}[{k}]: {t.numel()} values on {t.device}, data[{k}] has {w.numel()} on {w.device}")
            blobs[k] = _lib.SolverBlob(w.data_ptr(), g.data_ptr(), h0.data_ptr(), h1.data_ptr() if h1 is not None else None, w.numel(),
                                       lr_mults[k], decay_mults[k])
        L = _lib.lib()
        nbytes = L.fn2_solver_table_bytes(n, blobs)
        if nbytes == 0:
            check(-1)                                                                   # the library has recorded why
        self.tensors = (list(data), list(diff), list(hist0), hist1)
        self.ptrs = self.addresses(*self.tensors)
        self.nblobs = n
        self.device = data[0].device
        self.buffer = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.info = _lib.SolverTableInfo()
        with torch.cuda.device(self.device):
            check(L.fn2_solver_table_build(n, blobs, _ptr(self.buffer), nbytes, C.byref(self.info), _stream()))

    @staticmethod
    def addresses(data, diff, hist0, hist1=None):
        hist1 = hist1 if hist1 is not None else [None] * len(data)
        return tuple(t.data_ptr() if t is not None else 0 for group in (data, diff, hist0, hist1) for t in group)

    def matches(self, data, diff, hist0, hist1=None) -> bool:
        """Whether the table still describes these tensors (none has moved since the build: no Reshape, no re-assigned .data / .grad)."""
        return self.addresses(data, diff, hist0, hist1) == self.ptrs

    @property
    def nchunks(self) -> int:
        return int(self.info.nchunks)


def solver_apply_update(table: SolverTable, params: "_lib.SolverParams", rate: float, correction: float = 1.0, write_update: bool = False):
    """One fn2_solver_apply_update on the current stream: every blob of `table` in one launch (three with clipping); no host readback."""
    with torch.cuda.device(table.device):
        check(_lib.lib().fn2_solver_apply_update(C.byref(params), _ptr(table.buffer), C.byref(table.info), float(rate), float(correction),
                                                 int(bool(write_update)), _stream()))
