"""Thin torch-tensor front-ends of the C-ABI entry points (device pointers + current stream).

torch is used here for device memory and streams only; every computation is a HIP kernel of
libipsr_hip.so.  All functions require CUDA(HIP) tensors and raise otherwise — no fallback.
"""
import contextlib
import ctypes
import threading
import weakref
from collections import namedtuple

import torch

from . import _lib

_ws_cache = {}


def _stream():
    """The raw hipStream_t of torch's current stream on the current device (the C getter: no Stream object per launch)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _workspace(nbytes, device):
    """Grow-only per-(device, stream) scratch buffer; kernels on one stream run in order, so reuse is safe."""
    key = (device.index, _stream())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _empty(shape, dtype, device):
    """Every result, cache and ticket buffer of this module is allocated here or in `_zeros` (scratch comes from `_workspace`):
    the seams tests replace to place each buffer between guard bands (tests/guarded.py)."""
    return torch.empty(shape, dtype=dtype, device=device)


def _zeros(shape, dtype, device):
    return torch.zeros(shape, dtype=dtype, device=device)


def _on_current_device(t, name):
    # the kernels are launched on the CURRENT device's stream with raw pointers: a tensor living on another GPU would fault
    if t.device.index != torch._C._cuda_getDevice():        # (the C getter: this check runs ~700 times per training step)
        raise RuntimeError("%s is on %s but the current device is cuda:%d — wrap the call in torch.cuda.device(...) "
                           "(one process per GPU sets it once)" % (name, t.device, torch.cuda.current_device()))


def _req(t, dtype, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA/HIP tensor — the IPSR layer has no CPU path" % name)
    _on_current_device(t, name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def feat_mask_out_dim(n, layers=3):
    for _ in range(layers):
        n = (n + 2 - 4) // 2 + 1
    return n


def feat_mask(mask_hw, layers, threshold):
    """K1.  mask_hw: [H,W] bool/uint8 CUDA tensor -> [h,w] uint8."""
    m = mask_hw
    if m.dtype == torch.bool:
        m = m.to(torch.uint8)
    m = _req(m, torch.uint8, "mask")
    H, W = m.shape
    out = _empty((feat_mask_out_dim(H, layers), feat_mask_out_dim(W, layers)), dtype=torch.uint8, device=m.device)
    L = _lib.lib()
    nbytes = L.ipsr_feat_mask_workspace_bytes(H, W, layers)
    ws = _workspace(nbytes, m.device)
    _lib.check(L.ipsr_feat_mask(m.data_ptr(), H, W, layers, float(threshold), out.data_ptr(), ws.data_ptr(),
                                ws.numel(), _stream()), "ipsr_feat_mask")
    return out


def index_prep(feat_hw, patch, stride, mask_thred):
    """K2.  feat_hw [h,w] uint8 -> (flag [N] i32, mask_point_idx [N] i32 (first M valid), count [1] i32)."""
    f = _req(feat_hw, torch.uint8, "feature mask")
    h, w = f.shape
    n = ((h - patch) // stride + 1) * ((w - patch) // stride + 1)
    flag = _empty(n, dtype=torch.int32, device=f.device)
    mpi = _empty(n, dtype=torch.int32, device=f.device)
    cnt = _empty(1, dtype=torch.int32, device=f.device)
    _lib.check(_lib.lib().ipsr_index_prep(f.data_ptr(), h, w, patch, stride, int(mask_thred), flag.data_ptr(),
                                          mpi.data_ptr(), cnt.data_ptr(), _stream()), "ipsr_index_prep")
    return flag, mpi, cnt


def mask_index(masks, layers, threshold, patch, stride, mask_thred):
    """K1 + K2 for a batch of masks in ONE launch.  masks [R,H,W] (or [H,W]: R = 1) bool/uint8 -> (feat [R,h,w] u8, flag [R,N] i32,
    mask_point_idx [R,N] i32 (row r: first counts[r] valid, -1 after them), counts [R] i32), every row what `feat_mask` followed by
    `index_prep` gives for that mask.  layers == 0: `masks` are feature masks already, only the index part runs and feat is None."""
    m = masks
    if torch.is_tensor(m) and m.dtype == torch.bool:
        m = m.to(torch.uint8)
    m = _req(m, torch.uint8, "masks")
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3:
        raise RuntimeError("mask_index: masks must be [R,H,W] or [H,W], got %s" % (tuple(m.shape),))
    R, H, W = m.shape
    layers, patch, stride = int(layers), int(patch), int(stride)
    h, w = feat_mask_out_dim(H, layers), feat_mask_out_dim(W, layers)
    n = max((h - patch) // stride + 1, 0) * max((w - patch) // stride + 1, 0) if patch >= 1 and stride >= 1 else 0
    feat = _empty((R, max(h, 0), max(w, 0)), dtype=torch.uint8, device=m.device) if layers > 0 else None
    flag = _empty((R, n), dtype=torch.int32, device=m.device)
    mpi = _empty((R, n), dtype=torch.int32, device=m.device)
    cnt = _empty(R, dtype=torch.int32, device=m.device)
    L = _lib.lib()
    ws = _workspace(L.ipsr_mask_index_workspace_bytes(R, H, W, layers), m.device)
    _lib.check(L.ipsr_mask_index(m.data_ptr(), R, H, W, layers, float(threshold), patch, stride, int(mask_thred),
                                 feat.data_ptr() if feat is not None else None, flag.data_ptr(), mpi.data_ptr(), cnt.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream()), "ipsr_mask_index")
    return feat, flag, mpi, cnt


def patch_normalize(x_bcn):
    """K3.  x [B,C,N] -> (xn [B,C,N], inv [B,N])."""
    x = _req(x_bcn, torch.float32, "x")
    B, C, N = x.shape
    xn = _empty(x.shape, x.dtype, x.device)
    inv = _empty((B, N), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().ipsr_patch_normalize(x.data_ptr(), B, C, N, xn.data_ptr(), inv.data_ptr(), _stream()),
               "ipsr_patch_normalize")
    return xn, inv


def corr_argmax(xn_bcn, ref_bcn, want_S=False, corr="fp32"):
    """K4+K5.  -> (ind [B,N] i32, vmax [B,N], S [B,N,N] or None).
    corr="bf16": the opt-in bf16-MFMA kernel (operands rounded to bf16, fp32 accumulate); S is not available there."""
    xn = _req(xn_bcn, torch.float32, "xn")
    ref = _req(ref_bcn, torch.float32, "ref")
    B, C, N = xn.shape
    ind = _empty((B, N), dtype=torch.int32, device=xn.device)
    vmax = _empty((B, N), dtype=torch.float32, device=xn.device)
    if corr == "bf16":
        if want_S:
            raise ValueError("corr_argmax: the bf16 kernel does not materialise S")
        L = _lib.lib()
        ws = _workspace(L.ipsr_corr_argmax_bf16_workspace_bytes(B, C, N), xn.device)
        _lib.check(L.ipsr_corr_argmax_bf16(xn.data_ptr(), ref.data_ptr(), B, C, N, ind.data_ptr(), vmax.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream()), "ipsr_corr_argmax_bf16")
        return ind, vmax, None
    if corr != "fp32":
        raise ValueError("corr must be 'fp32' or 'bf16'")
    S = _empty((B, N, N), dtype=torch.float32, device=xn.device) if want_S else None
    L = _lib.lib()
    ws = _workspace(L.ipsr_corr_argmax_workspace_bytes(B, C, N), xn.device)
    _lib.check(L.ipsr_corr_argmax(xn.data_ptr(), ref.data_ptr(), B, C, N, ind.data_ptr(), vmax.data_ptr(),
                                  S.data_ptr() if want_S else None, ws.data_ptr(), ws.numel(), _stream()),
               "ipsr_corr_argmax")
    return ind, vmax, S


Forward = namedtuple("Forward", ["out", "ind", "vmax", "attn_rows", "bwd_index"])


_precision = threading.local()


@contextlib.contextmanager
def corr_precision(corr):
    """`with ops.corr_precision("bf16"):` — layer forwards issued by this thread inside the block run their correlation on
    the bf16 MFMA kernel (BASELINE config 5), for every shift_sz (p > 1: the 1x1 correlation under the fp32 window sums).
    The autograd surface IPSRFunction.apply has the reference's fixed 12 arguments, so the choice travels this way
    (IPSR_model sets it from its `corr_bf16` attribute)."""
    if corr not in ("fp32", "bf16"):
        raise ValueError("corr must be 'fp32' or 'bf16'")
    prev = getattr(_precision, "corr", "fp32")
    _precision.corr = corr
    try:
        yield
    finally:
        _precision.corr = prev


def forward(x, ref, mask_point_idx_i32, patch=1, stride=1, want_attn=False, want_index=True, corr=None, counts=None):
    """Whole layer forward.  x, ref [B,C,h,w] fp32; mask_point_idx_i32 [M] i32 -> Forward.
    want_attn:  also materialise the dense attention rows [B,M,N] (the reference's `in_attention`; tests and
                inspection only — the layer itself works on the compressed form);
    want_index: build the sparse trunc(kbar) the backward needs (skip under no_grad);
    corr:       "fp32" (the reference's arithmetic, default) or "bf16" (opt-in bf16-MFMA correlation; C % 64 == 0, and for
                patch == 1 N % 128 == 0, else NotImplementedError); None = what the enclosing `corr_precision` block says;
    counts:     [B] int32 DEVICE tensor = masked positions per sample (ipsr_forward_masks).  mask_point_idx is then [Mcap]
                (one index shared by the batch, e.g. straight from `index_prep`, no host sync) or [B,Mcap] (one row per
                sample: per-sample masks); entries past counts[b] are ignored.  Everything sized by M (attn_rows, bwd_index)
                is sized by the capacity Mcap; pass M = Mcap to `backward`."""
    if corr is None:
        corr = getattr(_precision, "corr", "fp32")
    if corr not in ("fp32", "bf16"):
        raise ValueError("corr must be 'fp32' or 'bf16'")
    x = _req(x, torch.float32, "input")
    ref = _req(ref, torch.float32, "ref.relu4_3")
    B, C, h, w = x.shape
    if tuple(ref.shape) != (B, C, h, w):
        raise RuntimeError("ref.relu4_3 %s does not match input %s" % (tuple(ref.shape), tuple(x.shape)))
    if stride != 1:
        raise NotImplementedError("IPSR layer: stride=%d is not implemented (only stride 1)" % stride)
    if patch < 1 or h < patch or w < patch:
        raise RuntimeError("IPSR layer: shift_sz=%d does not fit a %dx%d feature" % (patch, h, w))
    N = (h - patch + 1) * (w - patch + 1)       # window grid; = h*w for the reference's shift_sz = 1
    mpi = _req(mask_point_idx_i32, torch.int32, "mask_point_idx")
    if counts is not None:
        counts = _req(counts, torch.int32, "counts")
        if counts.numel() != B or mpi.dim() not in (1, 2) or (mpi.dim() == 2 and mpi.size(0) != B):
            raise RuntimeError("forward: counts must be [B] and mask_point_idx [Mcap] or [B,Mcap] (got %s, %s)" % (tuple(counts.shape), tuple(mpi.shape)))
        M = int(mpi.size(-1))
        if M < 1 or M > N:
            raise RuntimeError("forward: index capacity %d outside [1, %d]" % (M, N))
    else:
        M = int(mpi.numel())
    L = _lib.lib()
    dev = x.device
    out = _empty(x.shape, x.dtype, x.device)
    ind = _empty((B, N), dtype=torch.int32, device=dev)
    vmax = _empty((B, N), dtype=torch.float32, device=dev)
    attn = _empty((B, M, N), dtype=torch.float32, device=dev) if (want_attn and M > 0) else None
    bidx = _empty((B, L.ipsr_bwd_index_ints(N, M)), dtype=torch.int32, device=dev) if want_index else None
    bf = corr == "bf16"
    nbytes = (L.ipsr_forward_bf16corr_workspace_bytes if bf else L.ipsr_forward_workspace_bytes)(B, C, h, w, M, patch, stride)
    ws = _workspace(nbytes, dev)
    if counts is not None:
        _lib.check(L.ipsr_forward_masks(x.data_ptr(), ref.data_ptr(), mpi.data_ptr(), M if mpi.dim() == 2 else 0, counts.data_ptr(), M,
                                        B, C, h, w, patch, stride, out.data_ptr(), ind.data_ptr(), vmax.data_ptr(),
                                        attn.data_ptr() if attn is not None else None,
                                        bidx.data_ptr() if bidx is not None else None, ws.data_ptr(), ws.numel(), _stream(), int(bf)),
                   "ipsr_forward_masks")
        return Forward(out, ind, vmax, attn, bidx)
    _lib.check((L.ipsr_forward_bf16corr if bf else L.ipsr_forward)(
        x.data_ptr(), ref.data_ptr(), mpi.data_ptr() if M else None, M, B, C, h, w,
        patch, stride, out.data_ptr(), ind.data_ptr(), vmax.data_ptr(),
        attn.data_ptr() if attn is not None else None,
        bidx.data_ptr() if bidx is not None else None, ws.data_ptr(), ws.numel(), _stream()),
        "ipsr_forward_bf16corr" if bf else "ipsr_forward")
    if want_attn and attn is None:
        attn = _empty((B, 0, N), dtype=torch.float32, device=dev)
    return Forward(out, ind, vmax, attn, bidx)


def window_corr_plan(B, h, w, patch):
    """How the window arg-max of a shift_sz = `patch` forward would run (ipsr_window_corr_plan; host only, follows
    ipsr_debug_set_option(8, v)) -> {"variant": 0 streaming / 1 LDS-tiled, "workgroups", "split", "lds_bytes"}."""
    out = (ctypes.c_int * 4)()
    _lib.check(_lib.lib().ipsr_window_corr_plan(int(B), int(h), int(w), int(patch), ctypes.cast(out, ctypes.c_void_p)), "ipsr_window_corr_plan")
    return {"variant": out[0], "workgroups": out[1], "split": out[2], "lds_bytes": out[3]}


def backward(grad_out, bwd_index, triple_w, M, patch=1):
    """grad_in = g + triple_w * trunc(kbar)^T-weighted g; needs only the sparse index built by forward.
    patch > 1: the extension described at ipsr_backward_patch (include/ipsr_hip.h)."""
    g = _req(grad_out, torch.float32, "grad_output")
    B, C, h, w = g.shape
    gin = _empty(g.shape, g.dtype, g.device)
    L = _lib.lib()
    if patch == 1:
        _lib.check(L.ipsr_backward(g.data_ptr(), None, int(M), None, bwd_index.data_ptr(), float(triple_w),
                                   B, C, h, w, gin.data_ptr(), _stream()), "ipsr_backward")
    else:
        ws = _workspace(L.ipsr_backward_workspace_bytes(B, C, h, w, patch), g.device)
        _lib.check(L.ipsr_backward_patch(g.data_ptr(), int(M), bwd_index.data_ptr(), float(triple_w), B, C, h, w, int(patch),
                                         gin.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ipsr_backward_patch")
    return gin


def _act(t, name):
    """Activation operand of the glue and convolution kernels: contiguous fp32 or bf16 on the current device -> (tensor, is_bf16)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA/HIP tensor" % name)
    _on_current_device(t, name)
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("%s must be float32 or bfloat16, got %s" % (name, t.dtype))
    return (t if t.is_contiguous() else t.contiguous()), t.dtype == torch.bfloat16


def _f32(t):
    """bias / gamma / beta are fp32 parameters."""
    return None if t is None else _req(t, torch.float32, "parameter")


def bias_act_(x, bias, act="relu", slope=0.2, relu_into=None, relu_at=0, tickets=None):
    """In place x[b,c,...] = act(x + bias[c]) on a contiguous fp32/bf16 [B,C,*] tensor.  act: none | relu | leaky.
    relu_into / relu_at: a contiguous [B,Ctot,H,W] tensor whose channels [relu_at, relu_at + C) also receive relu(x + bias) — the skip
    half of the child level's concatenated tensor.  tickets: an int32 [C] tensor this launch zeroes for `bias_act_backward`'s in-launch
    batch sum of the bias gradient (the arrival counters live in the caller's memory, one set per autograd node)."""
    if not x.is_contiguous():
        raise RuntimeError("bias_act_ works in place and needs a contiguous tensor")
    x, bf = _act(x, "x")
    B, C = x.shape[0], x.shape[1]
    hw = x.numel() // (B * C)
    if relu_into is None:
        _lib.check(_lib.lib().ipsr_bias_act(x.data_ptr(), _ptr(_f32(bias)), B, C, hw, ACT_CODE[act], float(slope), bf, _ptr(tickets), _stream()),
                   "ipsr_bias_act")
        return x
    y2p, y2bs = _wide_slot(relu_into, x, relu_at, C, hw, "bias_act_: `relu_into`")
    _lib.check(_lib.lib().ipsr_bias_act_skip(x.data_ptr(), _ptr(_f32(bias)), B, C, hw, ACT_CODE[act], float(slope), bf, y2p, y2bs, _ptr(tickets),
                                             _stream()), "ipsr_bias_act_skip")
    return x


ACT_CODE = {"none": 0, "relu": 1, "leaky": 2}
INSTNORM_MAX_PLANE = 65536       # planes above 16384 elements must be a multiple of 4 (csrc/instnorm.hip)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _slot(t, c0, hw):
    """(pointer to channel c0 of a contiguous [B,Ctot,H,W] tensor, its batch stride in elements)."""
    return t.data_ptr() + c0 * hw * t.element_size(), t.shape[1] * hw


def _check_wide(wide, x, what):
    if wide.dtype != x.dtype or not wide.is_contiguous() or wide.dim() != 4 or wide.shape[0] != x.shape[0] \
            or tuple(wide.shape[2:]) != tuple(x.shape[2:]) or wide.device != x.device:
        raise RuntimeError("%s %s does not extend %s along the channels" % (what, tuple(wide.shape), tuple(x.shape)))


def _wide_slot(wide, x, at, C, hw, what):
    """`_slot` of the channels [at, at + C) of `wide`, a contiguous tensor that extends x along the channels."""
    _check_wide(wide, x, what)
    if at < 0 or at + C > wide.shape[1]:
        raise RuntimeError("%s: channels [%d, %d) outside %s" % (what, at, at + C, tuple(wide.shape)))
    return _slot(wide, at, hw)


def instnorm_act_forward(x, bias, gamma, beta, eps, act, slope, into=None, into_at=0, relu_into=None, relu_at=0, return_tickets=False):
    """y = act(InstanceNorm(x + bias[c]) * gamma[c] + beta[c]) -> (y, mean [B*C], rstd [B*C]); x contiguous fp32 / bf16 [B,C,H,W].
    return_tickets: also return tickets [C] int32, the arrival counters of the backward's in-launch batch sums, zeroed by this
    launch — hand them to `instnorm_act_backward` together with the statistics (one set per autograd node, like `bias_act_`'s).
    into / into_at: a contiguous [B,Ctot,H,W] tensor whose channels [into_at, into_at + C) receive y (a skip concatenation written
    in place); the returned y is then `into` itself.  relu_into / relu_at: a second destination of the same kind that receives
    relu(normalised value) — the skip half of the CHILD level's concatenated tensor."""
    x, bf = _act(x, "x")
    B, C = x.shape[0], x.shape[1]
    hw = x.numel() // (B * C)
    # one allocation: mean [B*C] | rstd [B*C] | the C ticket words of the backward's in-launch batch sums, zeroed by this launch
    stats = _empty(2 * B * C + C, dtype=torch.float32, device=x.device)
    mean, rstd, tickets = stats[:B * C], stats[B * C:2 * B * C], stats[2 * B * C:].view(torch.int32)
    if into is None and relu_into is None:
        y = _empty(x.shape, x.dtype, x.device)
        _lib.check(_lib.lib().ipsr_instnorm_act_forward(x.data_ptr(), _ptr(_f32(bias)), _ptr(_f32(gamma)), _ptr(_f32(beta)), float(eps),
                                                        ACT_CODE[act], float(slope), B, C, hw, bf, y.data_ptr(), mean.data_ptr(),
                                                        rstd.data_ptr(), tickets.data_ptr(), _stream()), "ipsr_instnorm_act_forward")
        return (y, mean, rstd, tickets) if return_tickets else (y, mean, rstd)
    if into is not None:
        y, (yp, ybs) = into, _wide_slot(into, x, into_at, C, hw, "instnorm_act_forward: `into`")
    else:
        y = _empty(x.shape, x.dtype, x.device)
        yp, ybs = y.data_ptr(), C * hw
    y2p, y2bs = None, 0
    if relu_into is not None:
        y2p, y2bs = _wide_slot(relu_into, x, relu_at, C, hw, "instnorm_act_forward: `relu_into`")
    _lib.check(_lib.lib().ipsr_instnorm_act_forward_slice(x.data_ptr(), _ptr(_f32(bias)), _ptr(_f32(gamma)), _ptr(_f32(beta)), float(eps),
                                                          ACT_CODE[act], float(slope), B, C, hw, bf, yp, ybs, y2p, y2bs,
                                                          mean.data_ptr(), rstd.data_ptr(), tickets.data_ptr(), _stream()),
               "ipsr_instnorm_act_forward_slice")
    return (y, mean, rstd, tickets) if return_tickets else (y, mean, rstd)


def instnorm_act_backward(dy, y, x, bias, gamma, mean, rstd, act, slope, need_affine, need_bias, at=0, dy2=None, dy2_at=0, tickets=None):
    """-> (dx, dgamma [C] | None, dbeta [C] | None, dbias [C] | None).  dy and y may be WIDER than x along the channels (contiguous
    [B,Ctot,H,W]): their channels [at, at + C) are the operands (a skip concatenation and its gradient, read in place).  dy2 / dy2_at:
    the gradient of the relu'd second output of the forward (channels [dy2_at, dy2_at + C) of a wide tensor), added inside the kernel.
    tickets: the int32 [C] words `instnorm_act_forward(..., return_tickets=True)` returned (None: fresh zeroed words are allocated
    here; they are never looked up behind `mean` / `rstd`)."""
    x, bf = _act(x, "x")
    B, C = x.shape[0], x.shape[1]
    hw = x.numel() // (B * C)
    if tickets is None:
        tickets = _zeros(C, dtype=torch.int32, device=x.device)
    elif tickets.dtype != torch.int32 or tickets.numel() != C or not tickets.is_contiguous() or tickets.device != x.device:
        raise RuntimeError("instnorm_act_backward: `tickets` must be the contiguous int32 [%d] words of the forward on %s" % (C, x.device))
    tick = tickets.data_ptr()
    dy, _ = _act(dy.to(x.dtype), "grad_output")
    dx = _empty(x.shape, x.dtype, x.device)
    part = _empty((3, B, C), dtype=torch.float32, device=x.device)
    # the batch sums of the per-plane partials are written by the same launch (the last plane of each channel to finish)
    sums = _empty((3, C), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    if dy.shape[1] == C and y.shape[1] == C and dy2 is None:
        _lib.check(L.ipsr_instnorm_act_backward(dy.data_ptr(), y.data_ptr(), x.data_ptr(), _ptr(_f32(bias)), _ptr(_f32(gamma)),
                                                mean.data_ptr(), rstd.data_ptr(), ACT_CODE[act], float(slope), B, C, hw, bf,
                                                dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), part[2].data_ptr(),
                                                _ptr(sums), tick, _stream()), "ipsr_instnorm_act_backward")
    else:
        _check_wide(dy, x, "instnorm_act_backward: grad_output")
        _check_wide(y, x, "instnorm_act_backward: output")
        if at < 0 or at + C > dy.shape[1] or (y.shape[1] != C and y.shape[1] != dy.shape[1]):
            raise RuntimeError("instnorm_act_backward: channels [%d, %d) outside %s / %s" % (at, at + C, tuple(dy.shape), tuple(y.shape)))
        dyp, dybs = _slot(dy, at if dy.shape[1] != C else 0, hw)
        yp, ybs = _slot(y, at if y.shape[1] != C else 0, hw)
        d2p, d2bs = None, 0
        if dy2 is not None:
            dy2, _ = _act(dy2.to(x.dtype), "second grad_output")
            d2p, d2bs = _wide_slot(dy2, x, dy2_at, C, hw, "instnorm_act_backward: second grad_output")
        _lib.check(L.ipsr_instnorm_act_backward_slice(dyp, dybs, d2p, d2bs, yp, ybs, x.data_ptr(), _ptr(_f32(bias)),
                                                      _ptr(_f32(gamma)), mean.data_ptr(), rstd.data_ptr(), ACT_CODE[act], float(slope), B, C, hw, bf,
                                                      dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), part[2].data_ptr(),
                                                      _ptr(sums), tick, _stream()), "ipsr_instnorm_act_backward_slice")
    s = sums
    return dx, (s[0] if need_affine else None), (s[1] if need_affine else None), (s[2] if need_bias else None)


def bias_act_backward(dy, y, act, slope, need_bias, dy2=None, dy2_at=0, tickets=None):
    """dx = dy * act'(y) (+ dy2[:, dy2_at : dy2_at + C] * relu'(y): the gradient of bias_act_'s second output), dbias [C] | None.
    tickets: the int32 [C] tensor the forward `bias_act_` zeroed (None: fresh zeroed words are allocated here)."""
    dy, bf = _act(dy.to(y.dtype), "grad_output")
    B, C = y.shape[0], y.shape[1]
    hw = y.numel() // (B * C)
    dx = _empty(y.shape, y.dtype, y.device)
    part = _empty((B, C), dtype=torch.float32, device=y.device) if need_bias else None
    sums = _empty(C, dtype=torch.float32, device=y.device) if need_bias else None
    if need_bias and tickets is None:
        tickets = _zeros(C, dtype=torch.int32, device=y.device)
    if dy2 is None:
        _lib.check(_lib.lib().ipsr_bias_act_backward(dy.data_ptr(), y.data_ptr(), ACT_CODE[act], float(slope), B, C, hw, bf, dx.data_ptr(),
                                                     _ptr(part), _ptr(sums), _ptr(tickets), _stream()), "ipsr_bias_act_backward")
    else:
        dy2, _ = _act(dy2.to(y.dtype), "second grad_output")
        d2p, d2bs = _wide_slot(dy2, y, dy2_at, C, hw, "bias_act_backward: second grad_output")
        _lib.check(_lib.lib().ipsr_bias_act_backward_skip(dy.data_ptr(), d2p, d2bs, y.data_ptr(), ACT_CODE[act], float(slope), B, C, hw, bf,
                                                          dx.data_ptr(), _ptr(part), _ptr(sums), _ptr(tickets), _stream()),
                   "ipsr_bias_act_backward_skip")
    return dx, (sums if need_bias else None)


def cat_relu_forward(y, x):
    """relu(torch.cat([y, x], 1)) in one pass; y [B,C1,H,W], x [B,C2,H,W] contiguous, same fp32/bf16 dtype."""
    y, bf = _act(y, "y")
    x, bf2 = _act(x, "x")
    if bf != bf2 or y.shape[0] != x.shape[0] or y.shape[2:] != x.shape[2:]:
        raise RuntimeError("cat_relu: mismatched operands %s %s / %s %s" % (tuple(y.shape), y.dtype, tuple(x.shape), x.dtype))
    B, C1, C2 = y.shape[0], y.shape[1], x.shape[1]
    hw = y.numel() // (B * C1)
    out = _empty((B, C1 + C2) + tuple(y.shape[2:]), dtype=y.dtype, device=y.device)
    _lib.check(_lib.lib().ipsr_cat_relu_forward(y.data_ptr(), x.data_ptr(), B, C1, C2, hw, bf, out.data_ptr(), _stream()),
               "ipsr_cat_relu_forward")
    return out


def cat_relu_skip_half_(out, x):
    """out[:, C1:] = relu(x) for a contiguous out [B,C1+C2,H,W] whose first C1 channels are already written (instnorm_act_forward
    with `into`): the skip half of relu(torch.cat([y, x], 1))."""
    x, bf = _act(x, "x")
    out, bf2 = _act(out, "out")
    B, C2 = x.shape[0], x.shape[1]
    C1 = out.shape[1] - C2
    if bf != bf2 or out.shape[0] != B or C1 < 1 or out.shape[2:] != x.shape[2:]:
        raise RuntimeError("cat_relu_skip_half_: mismatched operands %s / %s" % (tuple(out.shape), tuple(x.shape)))
    hw = x.numel() // (B * C2)
    _lib.check(_lib.lib().ipsr_cat_relu_forward(None, x.data_ptr(), B, C1, C2, hw, bf, out.data_ptr(), _stream()), "ipsr_cat_relu_forward")
    return out


def cat_relu_backward(grad_out, out, C1, skip_half_only=False):
    """-> (dy [B,C1,..] | None, dx [B,C2,..]): the ReLU mask from `out`, the channel slices as contiguous tensors; skip_half_only: dy is
    not produced (its consumer reads grad_out's slice in place)."""
    g, bf = _act(grad_out.to(out.dtype), "grad_output")
    B, C = out.shape[0], out.shape[1]
    C2 = C - C1
    hw = out.numel() // (B * C)
    dy = None if skip_half_only else _empty((B, C1) + tuple(out.shape[2:]), dtype=out.dtype, device=out.device)
    dx = _empty((B, C2) + tuple(out.shape[2:]), dtype=out.dtype, device=out.device)
    _lib.check(_lib.lib().ipsr_cat_relu_backward(g.data_ptr(), out.data_ptr(), B, C1, C2, hw, bf, _ptr(dy), dx.data_ptr(), _stream()),
               "ipsr_cat_relu_backward")
    return dy, dx


def bias_relu_pool2(x, bias):
    """max_pool2d(relu(x + bias[c]), 2, 2) of a contiguous fp32 / bf16 [B,C,H,W] tensor in one pass (an odd last row / column is dropped)."""
    x, bf = _act(x, "x")
    B, C, H, W = x.shape
    y = _empty((B, C, H // 2, W // 2), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().ipsr_bias_relu_pool2(x.data_ptr(), _ptr(_f32(bias)), B, C, H, W, bf, y.data_ptr(), _stream()),
               "ipsr_bias_relu_pool2")
    return y


CONV_FWD, CONV_BWD_DATA, CONVT_FWD, CONVT_BWD_DATA = 0, 1, 2, 3

# arithmetic of the Winograd GEMMs (include/ipsr_hip.h, ipsr_conv3x3_winograd_mp): "fp32" = fp32 operands on the fp32 MFMA (the
# reference's arithmetic, default); "bf16x3" / "bf16x6" = transformed operands split into 2 / 3 bf16 numbers, multiplied on the bf16
# MFMA with fp32 accumulation (error ~1e-4 / ~1e-5 of the output scale; a plain bf16 convolution: ~2e-3).
#
# The four opt-in "direct" names (fp32 activations only) are no Winograd arithmetic: the Winograd engines keep fp32 (code 0) under them,
# and the dispatcher (models/hipconv.py) moves the passes named here to the DIRECT kernels on split-bf16 operands (csrc/conv_bf16.hip:
# every operand hi + lo, every product lo*hi + hi*lo + hi*hi, fp32 accumulation, error ~6e-6), wherever the kernel takes the shape:
#   "k3_data"  forward / input gradient of the k3 s1 p1 layers that "winograd" has               -> conv3x3_bf16x3      (engine "bf16x3d")
#   "k3_wrw"   weight gradient of the k3 s1 p1 layers of that row of hipconv._DIRECT_OPT_INS     -> conv3x3_bf16x3_wrw  (engine "bf16x3w")
#   "s2_data"  forward / input gradient of the k4 s2 p1 layers of that row                       -> conv4x4s2_bf16x3   (engine "bf16x3d")
#   "s2_wrw"   weight gradient of the k4 s2 p1 layers of that row                                -> conv4x4s2_bf16x3_wrw (engine "bf16x3w")
# Each name moves what the one before it moves, plus one more pass.  This table is the one place that says so.
DIRECT_PASSES = {
    "direct_bf16x3": frozenset({"k3_data"}),
    "direct_bf16x3_dw": frozenset({"k3_data", "k3_wrw"}),
    "direct_bf16x3_s2": frozenset({"k3_data", "k3_wrw", "s2_data"}),
    "direct_bf16x3_s2_dw": frozenset({"k3_data", "k3_wrw", "s2_data", "s2_wrw"}),
}
MATH_CODE = {None: 0, "fp32": 0, "bf16x3": 2, "bf16x6": 3, **dict.fromkeys(DIRECT_PASSES, 0)}


def direct_moves(math, which):
    """True when the arithmetic name `math` moves the pass `which` (a key of DIRECT_PASSES' sets) to the direct split-bf16 kernels."""
    return which in DIRECT_PASSES.get(math, ())


def _io_code(in_bf16, out_dtype):
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("out_dtype must be float32 or bfloat16")
    return int(bool(in_bf16)) | (2 if out_dtype == torch.bfloat16 else 0)


def _data_pass_shapes(op, in_shape, Cout, k, out_hw):
    """-> (input, weight, result) shapes of a forward / input-gradient pass in the MODULE's terms: `in_shape` = (B, Cin, H, W) of the
    module's input whatever the op, out_hw = (Ho, Wo) of its output; the pass reads x (forward ops) or dy (backward-data ops)."""
    B, Cin, H, W = in_shape
    xs, ys = (B, Cin, H, W), (B, Cout) + out_hw
    wsh = (Cout, Cin, k, k) if op in (CONV_FWD, CONV_BWD_DATA) else (Cin, Cout, k, k)
    return (xs, wsh, ys) if op in (CONV_FWD, CONVT_FWD) else (ys, wsh, xs)


def _result(out, shape, dtype, device, what):
    """The tensor a front-end writes: a fresh one, or the caller's `out` (e.g. a slice of a gradient bucket) once it is checked."""
    if out is None:
        return _empty(shape, dtype, device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous() or out.device != device:
        raise RuntimeError("%s: `out` must be a contiguous %s %s tensor on %s" % (what, dtype, tuple(shape), device))
    return out


def _probed_workspace(L, nbytes, device, what, args):
    """The scratch buffer for the answer `nbytes` of a workspace query; 0 = the library does not implement the shape (`what % args`)."""
    if nbytes == 0:
        raise NotImplementedError("%s is not implemented: %s" % (what % args, L.ipsr_last_error().decode("utf-8", "replace")))
    return _workspace(nbytes, device)


def conv_out_dim(op, n, k, stride, pad, dil):
    if op in (CONV_FWD, CONV_BWD_DATA):
        return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return (n - 1) * stride - 2 * pad + dil * (k - 1) + 1


def conv2d_supported(op, B, Cin, H, W, Cout, k, stride, pad, dil):
    """True when ipsr_conv2d implements this geometry (its workspace query answers 0 otherwise)."""
    return _lib.lib().ipsr_conv2d_workspace_bytes(op, B, Cin, H, W, Cout, k, stride, pad, dil) > 0


def conv2d(op, inp, weight, in_shape, Cout, k, stride, pad, dil):
    """The bias-free convolution kernels (include/ipsr_hip.h, ipsr_conv2d).  `in_shape` = (B, Cin, H, W) of the MODULE's input
    whatever the op; `inp` is x for the forward ops and dy for the backward-data ops.  Returns y / dx (fp32, contiguous)."""
    B, Cin, H, W = in_shape
    Ho, Wo = conv_out_dim(op, H, k, stride, pad, dil), conv_out_dim(op, W, k, stride, pad, dil)
    inp = _req(inp, torch.float32, "conv input")
    weight = _req(weight, torch.float32, "conv weight")
    want_in, want_w, oshape = _data_pass_shapes(op, in_shape, Cout, k, (Ho, Wo))
    if tuple(inp.shape) != want_in or tuple(weight.shape) != want_w:
        raise RuntimeError("conv2d op %d: input %s / weight %s do not match %s / %s" % (op, tuple(inp.shape), tuple(weight.shape), want_in, want_w))
    out = _empty(oshape, dtype=torch.float32, device=inp.device)
    L = _lib.lib()
    ws = _probed_workspace(L, L.ipsr_conv2d_workspace_bytes(op, B, Cin, H, W, Cout, k, stride, pad, dil), inp.device,
                           "ipsr_conv2d: op %d with k=%d stride=%d pad=%d dil=%d, Cin=%d Cout=%d", (op, k, stride, pad, dil, Cin, Cout))
    _lib.check(L.ipsr_conv2d(op, inp.data_ptr(), weight.data_ptr(), out.data_ptr(), B, Cin, H, W, Cout, k, stride, pad, dil,
                             ws.data_ptr(), ws.numel(), _stream()), "ipsr_conv2d")
    return out


def winograd_supported(op, B, Cin, H, W, Cout):
    return _lib.lib().ipsr_conv3x3_winograd_workspace_bytes(op, B, Cin, H, W, Cout) > 0


_EPILOGUE = {None: 0, "none": 0, "relu": 1, "relu_pool": 2}


def winograd_filter_cache(op, Cin, Cout, device):
    """An empty buffer for the transformed filter of one layer (see conv3x3_winograd's `filter_cache`)."""
    n = _lib.lib().ipsr_conv3x3_winograd_filter_floats(op, Cin, Cout)
    return _empty(n, dtype=torch.float32, device=device)


def conv3x3_winograd(op, inp, weight, in_shape, Cout, bias=None, epilogue=None, filter_cache=None, filter_cache_valid=False,
                     math=None, out_dtype=None):
    """k3 s1 p1 convolution / transposed convolution / their input gradients by Winograd F(4x4,3x3) (ipsr_conv3x3_winograd_mp).
    epilogue: None | "relu" (out = relu(conv + bias)) | "relu_pool" (... followed by the 2x2 max-pool; output [.,.,H/2,W/2]);
    filter_cache: buffer from `winograd_filter_cache`; the transformed filter is written into it unless filter_cache_valid (a
    cache is only valid for the `math` it was filled under);
    math: see MATH_CODE; inp may be fp32 or bf16, out_dtype (default: inp's dtype) likewise."""
    B, Cin, H, W = in_shape
    inp, in_bf = _act(inp, "conv input")
    weight = _req(weight, torch.float32, "conv weight")
    out_dtype = out_dtype or inp.dtype
    fwd = op in (CONV_FWD, CONVT_FWD)
    want_in, want_w, oshape = _data_pass_shapes(op, in_shape, Cout, 3, (H, W))
    if tuple(inp.shape) != want_in or tuple(weight.shape) != want_w:
        raise RuntimeError("conv3x3_winograd op %d: input %s / weight %s do not match %s / %s" % (op, tuple(inp.shape), tuple(weight.shape), want_in, want_w))
    epi = _EPILOGUE[epilogue]
    if epi and not fwd:
        raise ValueError("conv3x3_winograd: an epilogue only makes sense on a forward op")
    if epi == 2 and (H % 2 or W % 2):
        raise RuntimeError("conv3x3_winograd: relu_pool needs even extents, got %dx%d" % (H, W))
    out = _empty((B, Cout, H // 2, W // 2) if epi == 2 else oshape, dtype=out_dtype, device=inp.device)      # (an epilogue: a forward op)
    L = _lib.lib()
    ws = _probed_workspace(L, L.ipsr_conv3x3_winograd_workspace_bytes(op, B, Cin, H, W, Cout), inp.device, "ipsr_conv3x3_winograd: op %d Cin=%d Cout=%d", (op, Cin, Cout))
    if filter_cache is not None and filter_cache.numel() != L.ipsr_conv3x3_winograd_filter_floats(op, Cin, Cout):
        raise RuntimeError("conv3x3_winograd: filter_cache has the wrong size")
    _lib.check(L.ipsr_conv3x3_winograd_mp(op, inp.data_ptr(), weight.data_ptr(), _ptr(_f32(bias)), epi, _ptr(filter_cache),
                                          int(bool(filter_cache_valid)), out.data_ptr(), B, Cin, H, W, Cout, MATH_CODE[math], _io_code(in_bf, out_dtype),
                                          ws.data_ptr(), ws.numel(), _stream()), "ipsr_conv3x3_winograd_mp")
    return out


# ---- the direct kernels of csrc/conv_bf16.hip: one implementation per pass shape.  `arith` = "bf16" (bf16 activations in, bf16 or fp32 out:
# BASELINE config 5) or "bf16x3" (fp32 in and out, operands split into hi + lo in the kernel); it is also the part of the public functions'
# and of the C entries' names that differs, so every message names the function the caller used.

def _direct_operands(arith, who, *named):
    """The activation operands (tensor, name, ...) of a direct pass: all bf16 under "bf16", all fp32 under "bf16x3"."""
    if arith.startswith("bf16x3"):
        return [_req(t, torch.float32, name) for t, name in zip(named[::2], named[1::2])]
    acts = [_act(t, name) for t, name in zip(named[::2], named[1::2])]
    if not all(bf for _, bf in acts):
        raise TypeError("%s reads bf16 %s" % (who, "tensors" if len(acts) > 1 else "activations, got %s" % acts[0][0].dtype))
    return [t for t, _ in acts]


# frozen weights: weight tensor (weakly held) -> {key: ((version, data pointer), shape, buffer holding the re-packed bf16 weights)}.  Keyed by
# the tensor OBJECT (the module's Parameter, `pack_key`): a storage pointer comes back to life with another tensor's data once the first is
# freed (two test cases with equal shapes met that way).  (id-keyed with a weak reference for liveness: tensors compare elementwise, which
# rules out a WeakKeyDictionary)
_BF16_PACKS = {}
# conv3x3_bf16 / conv3x3_bf16x3 calls that ran the weight-packing launch (a cache miss, or no cache asked for): what tests count the cache's hits by
bf16_pack_launches = 0


def _packs_of(weight):
    ent = _BF16_PACKS.get(id(weight))
    if ent is None or ent[0]() is not weight:
        key = id(weight)
        ent = (weakref.ref(weight, lambda _r, key=key: _BF16_PACKS.pop(key, None)), {})
        _BF16_PACKS[key] = ent
    return ent[1]


def _pack_workspace(weight, pack_key, key, nbytes, device, keep_packed):
    """-> (workspace, valid) of a 3x3 data pass.  keep_packed: the packed weights live in a buffer of their own, cached under the tensor
    object `pack_key` (default `weight`) and `key`; valid = 1 when it already holds this weight's image (same version counter, data
    pointer and shape), so the packing launch is skipped.  Otherwise the shared scratch buffer, packed on every call."""
    global bf16_pack_launches
    valid = 0
    if keep_packed:
        packs = _packs_of(weight if pack_key is None else pack_key)
        ent = packs.get(key)
        if ent is not None and ent[0] == (weight._version, weight.data_ptr()) and ent[1] == tuple(weight.shape) and ent[2].numel() >= nbytes \
                and ent[2].device == device:
            ws, valid = ent[2], 1
        else:
            ws = _empty(nbytes, dtype=torch.uint8, device=device)
            packs[key] = ((weight._version, weight.data_ptr()), tuple(weight.shape), ws)
    else:
        ws = _workspace(nbytes, device)
    bf16_pack_launches += 1 - valid
    return ws, valid


def _conv3x3_direct(arith, op, inp, weight, in_shape, Cout, out_dtype, keep_packed, pack_key):
    who, x3 = "conv3x3_" + arith, arith == "bf16x3"
    B, Cin, H, W = in_shape
    inp, = _direct_operands(arith, who, inp, "conv input")
    weight = _req(weight, torch.float32, "conv weight")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("%s writes bf16 or fp32, not %s" % (who, out_dtype))
    want_in, want_w, oshape = _data_pass_shapes(op, in_shape, Cout, 3, (H, W))
    if tuple(inp.shape) != want_in or tuple(weight.shape) != want_w:
        raise RuntimeError("%s op %d: input %s / weight %s do not match %s / %s" % (who, op, tuple(inp.shape), tuple(weight.shape), want_in, want_w))
    L = _lib.lib()
    nbytes = getattr(L, "ipsr_conv3x3_%s_workspace_bytes" % arith)(op, B, Cin, H, W, Cout)
    if nbytes == 0:
        raise NotImplementedError("ipsr_conv3x3_bf16%s: op %d on %s is not implemented (%s)" % (" (io 2)" if x3 else "", op, (B, Cin, H, W, Cout), L.ipsr_last_error().decode("utf-8", "replace")))
    out = _empty(oshape, dtype=out_dtype, device=inp.device)
    ws, valid = _pack_workspace(weight, pack_key, ("x3", op) if x3 else op, nbytes, inp.device, keep_packed)
    _lib.check(L.ipsr_conv3x3_bf16_packed(op, inp.data_ptr(), weight.data_ptr(), out.data_ptr(), B, Cin, H, W, Cout, 2 if x3 else int(out_dtype == torch.bfloat16),
                                          valid, ws.data_ptr(), ws.numel(), _stream()), "ipsr_conv3x3_bf16")
    return out


def _conv4x4s2_direct(arith, mode, inp, weight, B, Kc, Cf, nh, nw, out_dtype):
    who = "conv4x4s2_" + arith
    inp, = _direct_operands(arith, who, inp, "conv input")
    weight = _req(weight, torch.float32, "conv weight")
    if mode not in (_S2_X3_MODES if arith == "bf16x3" else _S2_MODES):
        raise ValueError("%s: mode %r" % (who, mode))
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("%s writes bf16 or fp32, not %s" % (who, out_dtype))
    fine, coarse = (B, Cf, 2 * nh, 2 * nw), (B, Kc, nh, nw)
    want_in, oshape = (fine, coarse) if mode & ~S2_DILATED == S2_FINE_TO_COARSE else (coarse, fine)
    if tuple(inp.shape) != want_in or tuple(weight.shape) != (Kc, Cf, 4, 4):
        raise RuntimeError("%s mode %d: input %s / weight %s do not match %s / %s" % (who, mode, tuple(inp.shape), tuple(weight.shape), want_in, (Kc, Cf, 4, 4)))
    L = _lib.lib()
    out = _empty(oshape, dtype=out_dtype, device=inp.device)
    ws = _probed_workspace(L, getattr(L, "ipsr_%s_workspace_bytes" % who)(mode, B, Kc, Cf, nh, nw), inp.device, "ipsr_" + who + ": mode %d on %s", (mode, (B, Kc, Cf, nh, nw)))
    io = () if arith == "bf16x3" else (int(out_dtype == torch.bfloat16),)          # ipsr_conv4x4s2_bf16x3 has no io code: fp32 in and out
    _lib.check(getattr(L, "ipsr_" + who)(mode, inp.data_ptr(), weight.data_ptr(), out.data_ptr(), B, Kc, Cf, nh, nw, *io, ws.data_ptr(), ws.numel(), _stream()),
               "ipsr_" + who)
    return out


def _conv4x4s2_direct_wrw(arith, fine, coarse, B, Kc, Cf, nh, nw, out):
    who = "conv4x4s2_%s_wrw" % arith
    fine, coarse = _direct_operands(arith, who, fine, "fine tensor", coarse, "coarse tensor")
    if tuple(fine.shape) != (B, Cf, 2 * nh, 2 * nw) or tuple(coarse.shape) != (B, Kc, nh, nw):
        raise RuntimeError("%s: fine %s / coarse %s do not match %s / %s" % (who, tuple(fine.shape), tuple(coarse.shape), (B, Cf, 2 * nh, 2 * nw), (B, Kc, nh, nw)))
    L = _lib.lib()
    dw = _result(out, (Kc, Cf, 4, 4), torch.float32, fine.device, who)
    ws = _probed_workspace(L, getattr(L, "ipsr_%s_workspace_bytes" % who)(B, Kc, Cf, nh, nw), fine.device, "ipsr_" + who + ": %s", ((B, Kc, Cf, nh, nw),))
    _lib.check(getattr(L, "ipsr_" + who)(fine.data_ptr(), coarse.data_ptr(), dw.data_ptr(), B, Kc, Cf, nh, nw, ws.data_ptr(), ws.numel(), _stream()),
               "ipsr_" + who)
    return dw


def _conv3x3_direct_wrw(arith, transposed, x, dy, Cout, out):
    who, x3 = "conv3x3_%s_wrw" % arith, arith == "bf16x3"
    x, dy = _direct_operands(arith, who, x, "conv input", dy, "grad_output")
    B, Cin, H, W = x.shape
    if tuple(dy.shape) != (B, Cout, H, W):
        raise RuntimeError("%s: grad_output %s does not match %s" % (who, tuple(dy.shape), (B, Cout, H, W)))
    L = _lib.lib()
    dw = _result(out, (Cin, Cout, 3, 3) if transposed else (Cout, Cin, 3, 3), torch.float32, x.device, who)
    ws = _probed_workspace(L, getattr(L, "ipsr_%s_workspace_bytes" % who)(int(transposed), B, Cin, H, W, Cout), x.device,
                           "ipsr_conv3x3_bf16_wrw%s: %%s" % (" (split-bf16)" if x3 else ""), ((B, Cin, H, W, Cout),))
    form = int(bool(transposed)) + (2 if x3 else 0)              # forms 0 / 1: bf16 operands, 2 / 3: fp32 operands split in the kernel
    _lib.check(L.ipsr_conv3x3_bf16_wrw(form, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, Cin, H, W, Cout, ws.data_ptr(), ws.numel(),
                                       _stream()), "ipsr_conv3x3_bf16_wrw")
    return dw


def conv3x3_bf16_supported(op, B, Cin, H, W, Cout):
    return _lib.lib().ipsr_conv3x3_bf16_workspace_bytes(op, B, Cin, H, W, Cout) > 0


def conv3x3_bf16(op, inp, weight, in_shape, Cout, out_dtype=torch.bfloat16, keep_packed=False, pack_key=None):
    """k3 s1 p1 convolution / transposed convolution / their input gradients as ONE direct implicit GEMM on the bf16 matrix cores
    (ipsr_conv3x3_bf16, csrc/conv_bf16.hip): bf16 activations in, bf16 or fp32 out, fp32 weights cast inside.  BASELINE config 5.
    keep_packed: the weights are FROZEN (VGG16): their re-packed bf16 image is kept and the packing launch skipped from the second
    call on.  The image is cached under the tensor object `pack_key` (default `weight`; pass the Parameter when `weight` is a
    detached view of it, which is a new object on every call) and is valid while the key's version counter and data pointer are
    unchanged.  Writes through `weight.data` are not seen: `.data` has a version counter of its own."""
    return _conv3x3_direct("bf16", op, inp, weight, in_shape, Cout, out_dtype, keep_packed, pack_key)


def conv3x3_bf16x3_supported(op, B, Cin, H, W, Cout):
    return _lib.lib().ipsr_conv3x3_bf16x3_workspace_bytes(op, B, Cin, H, W, Cout) > 0


def conv3x3_bf16x3(op, inp, weight, in_shape, Cout, keep_packed=False, pack_key=None):
    """k3 s1 p1 convolution / transposed convolution / their input gradients on FP32 tensors as ONE direct implicit GEMM on the bf16
    matrix cores with split operands (io code 2 of ipsr_conv3x3_bf16, csrc/conv_bf16.hip): every operand hi + lo, every product
    lo*hi + hi*lo + hi*hi, fp32 accumulation; fp32 in, fp32 out.  keep_packed / pack_key: as in conv3x3_bf16 (the hi and lo planes of
    the packed weights are kept; cached apart from the bf16 kernel's pack of the same weight)."""
    return _conv3x3_direct("bf16x3", op, inp, weight, in_shape, Cout, torch.float32, keep_packed, pack_key)


def conv4x4s2_bf16_supported(mode, B, Kc, Cf, nh, nw):
    return mode in (S2_FINE_TO_COARSE, S2_COARSE_TO_FINE) and _lib.lib().ipsr_conv4x4s2_bf16_workspace_bytes(mode, B, Kc, Cf, nh, nw) > 0


def conv4x4s2_bf16(mode, inp, weight, B, Kc, Cf, nh, nw, out_dtype=torch.bfloat16):
    """The k4 s2 p1 layers as ONE direct implicit GEMM on the bf16 matrix cores (ipsr_conv4x4s2_bf16), in the coarse / fine terms of
    conv4x4s2_winograd: mode S2_FINE_TO_COARSE: inp = fine [B,Cf,2nh,2nw] -> coarse [B,Kc,nh,nw]; S2_COARSE_TO_FINE: the reverse.
    weight [Kc,Cf,4,4] fp32 (Conv2d: [Cout,Cin]; ConvTranspose2d: [Cin,Cout])."""
    return _conv4x4s2_direct("bf16", mode, inp, weight, B, Kc, Cf, nh, nw, out_dtype)


def conv4x4s2_bf16_dil_supported(mode, B, Kc, Cf, nh, nw):
    return mode in _S2_MODES and _lib.lib().ipsr_conv4x4s2_bf16_dil_workspace_bytes(mode, B, Kc, Cf, nh, nw) > 0


def conv4x4s2_bf16_dil(mode, inp, weight, B, Kc, Cf, nh, nw, out_dtype=torch.bfloat16):
    """Conv2d(Cf, Kc, k4, stride 2, pad 3, dilation 2) on bf16 tensors as ONE direct implicit GEMM on the bf16 matrix cores
    (ipsr_conv4x4s2_bf16_dil), in the terms of conv4x4s2_bf16: S2_FINE_TO_COARSE its forward (inp = fine [B,Cf,2nh,2nw] -> coarse
    [B,Kc,nh,nw]; only the odd rows and odd columns of `inp` are used), S2_COARSE_TO_FINE its input gradient (every element of the fine
    result is written: the odd / odd quarter carries values, the rest is +0).  weight [Kc,Cf,4,4] fp32; bf16 or fp32 out."""
    return _conv4x4s2_direct("bf16_dil", mode, inp, weight, B, Kc, Cf, nh, nw, out_dtype)


def conv4x4s2_bf16x3_supported(mode, B, Kc, Cf, nh, nw):
    return mode in _S2_X3_MODES and _lib.lib().ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, B, Kc, Cf, nh, nw) > 0


def conv4x4s2_bf16x3(mode, inp, weight, B, Kc, Cf, nh, nw):
    """The k4 s2 p1 layers on FP32 tensors as ONE direct implicit GEMM on the bf16 matrix cores with split operands (ipsr_conv4x4s2_bf16x3,
    csrc/conv_bf16.hip): every operand hi + lo, every product lo*hi + hi*lo + hi*hi, fp32 accumulation; fp32 in, fp32 out.  mode, shapes
    and weight as in conv4x4s2_bf16.  With S2_DILATED or-ed into the mode the layer is Conv2d(k4, stride 2, pad 3, dilation 2) in the same
    terms: S2_DILATED | S2_FINE_TO_COARSE its forward, S2_DILATED | S2_COARSE_TO_FINE its input gradient (every element of the fine result
    is written: the odd / odd quarter carries values, the rest is zero)."""
    return _conv4x4s2_direct("bf16x3", mode, inp, weight, B, Kc, Cf, nh, nw, torch.float32)


def conv4x4s2_bf16_wrw_supported(B, Kc, Cf, nh, nw):
    return _lib.lib().ipsr_conv4x4s2_bf16_wrw_workspace_bytes(B, Kc, Cf, nh, nw) > 0


def conv4x4s2_bf16_wrw(fine, coarse, B, Kc, Cf, nh, nw, out=None):
    """Weight gradient [Kc,Cf,4,4] (fp32) of a k4 s2 p1 layer from its bf16 fine [B,Cf,2nh,2nw] and coarse [B,Kc,nh,nw] tensors
    (ipsr_conv4x4s2_bf16_wrw); `out`: optional contiguous fp32 destination (a gradient bucket slice)."""
    return _conv4x4s2_direct_wrw("bf16", fine, coarse, B, Kc, Cf, nh, nw, out)


def conv4x4s2_bf16x3_wrw_supported(B, Kc, Cf, nh, nw):
    return _lib.lib().ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(B, Kc, Cf, nh, nw) > 0


def conv4x4s2_bf16x3_wrw(fine, coarse, B, Kc, Cf, nh, nw, out=None):
    """Weight gradient [Kc,Cf,4,4] (fp32) of a k4 s2 p1 layer from its FP32 fine [B,Cf,2nh,2nw] and coarse [B,Kc,nh,nw] tensors on the bf16
    matrix cores with split operands (ipsr_conv4x4s2_bf16x3_wrw): every operand hi + lo, every product lo*hi + hi*lo + hi*hi, fp32
    accumulation, the split in the kernel; `out`: optional contiguous fp32 destination (a gradient bucket slice)."""
    return _conv4x4s2_direct_wrw("bf16x3", fine, coarse, B, Kc, Cf, nh, nw, out)


def conv4x4s2_bf16x3_dil_wrw_supported(B, Kc, Cf, nh, nw):
    return _lib.lib().ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(B, Kc, Cf, nh, nw) > 0


def conv4x4s2_bf16x3_dil_wrw(fine, coarse, B, Kc, Cf, nh, nw, out=None):
    """Weight gradient [Kc,Cf,4,4] (fp32) of Conv2d(Cf, Kc, k4, stride 2, pad 3, dilation 2) from its FP32 input fine [B,Cf,2nh,2nw] and
    output gradient coarse [B,Kc,nh,nw] on the bf16 matrix cores with split operands (ipsr_conv4x4s2_bf16x3_dil_wrw); arithmetic and `out`
    as in conv4x4s2_bf16x3_wrw."""
    return _conv4x4s2_direct_wrw("bf16x3_dil", fine, coarse, B, Kc, Cf, nh, nw, out)


def conv4x4s2_bf16_dil_wrw_supported(B, Kc, Cf, nh, nw):
    return _lib.lib().ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes(B, Kc, Cf, nh, nw) > 0


def conv4x4s2_bf16_dil_wrw(fine, coarse, B, Kc, Cf, nh, nw, out=None):
    """Weight gradient [Kc,Cf,4,4] (fp32) of Conv2d(Cf, Kc, k4, stride 2, pad 3, dilation 2) from its bf16 input fine [B,Cf,2nh,2nw] and bf16
    output gradient coarse [B,Kc,nh,nw] on the bf16 matrix cores (ipsr_conv4x4s2_bf16_dil_wrw): one MFMA per product, fp32 accumulation, only
    the odd rows and odd columns of `fine` are used; `out` as in conv4x4s2_bf16_wrw."""
    return _conv4x4s2_direct_wrw("bf16_dil", fine, coarse, B, Kc, Cf, nh, nw, out)


def conv3x3_bf16_wrw_supported(transposed, B, Cin, H, W, Cout):
    return _lib.lib().ipsr_conv3x3_bf16_wrw_workspace_bytes(int(transposed), B, Cin, H, W, Cout) > 0


def conv3x3_bf16_wrw(transposed, x, dy, Cout, out=None):
    """Weight gradient of a k3 s1 p1 Conv2d (-> [Cout,Cin,3,3]) / ConvTranspose2d (-> [Cin,Cout,3,3]) on the bf16 matrix cores
    (ipsr_conv3x3_bf16_wrw): x, dy bf16; the result fp32 (optionally written into `out`, e.g. a slice of a gradient bucket)."""
    return _conv3x3_direct_wrw("bf16", transposed, x, dy, Cout, out)


def conv3x3_bf16x3_wrw_supported(transposed, B, Cin, H, W, Cout):
    return _lib.lib().ipsr_conv3x3_bf16x3_wrw_workspace_bytes(int(transposed), B, Cin, H, W, Cout) > 0


def conv3x3_bf16x3_wrw(transposed, x, dy, Cout, out=None):
    """Weight gradient of a k3 s1 p1 Conv2d (-> [Cout,Cin,3,3]) / ConvTranspose2d (-> [Cin,Cout,3,3]) on FP32 tensors with split-bf16
    operands (forms 2 / 3 of ipsr_conv3x3_bf16_wrw): x, dy fp32; the result fp32 (optionally written into `out`, e.g. a slice of a
    gradient bucket)."""
    return _conv3x3_direct_wrw("bf16x3", transposed, x, dy, Cout, out)


GEOM_K4_S2_P3_D2 = 0       # Conv2d(k4, stride 2, pad 3, dilation 2): netG's down convolution
GEOM_K4_S1_P1 = 1          # Conv2d(k4, stride 1, pad 1): netD's fourth convolution


def conv4x4_geometry(k, stride, pad, dil):
    """-> the `geom` of ipsr_conv4x4_winograd for a Conv2d, or None."""
    if (k, stride, pad, dil) == (4, 2, 3, 2):
        return GEOM_K4_S2_P3_D2
    if (k, stride, pad, dil) == (4, 1, 1, 1):
        return GEOM_K4_S1_P1
    return None


def dilated_winograd_supported(mode, B, Cin, H, W, Cout, geom=GEOM_K4_S2_P3_D2):
    return _lib.lib().ipsr_conv4x4_winograd_workspace_bytes(geom, mode, B, Cin, H, W, Cout) > 0


def conv4x4_dilated_winograd(mode, a, b, in_shape, Cout, out=None, geom=GEOM_K4_S2_P3_D2, math=None, out_dtype=None):
    """Conv2d(k4, stride 2, pad 3, dilation 2) (geom 0) or Conv2d(k4, stride 1, pad 1) (geom 1) by Winograd F(3x3,4x4)
    (ipsr_conv4x4_winograd_mp): mode 0 forward (a = x, b = weight -> y), 1 backward-data (a = dy, b = weight -> dx), 2 weight
    gradient (a = x, b = dy -> dw, always fp32).  Activations fp32 or bf16; math: see MATH_CODE."""
    B, Cin, H, W = in_shape
    a, a_bf = _act(a, "operand a")
    if mode == 2:
        b, b_bf = _act(b, "operand b")
        if b_bf != a_bf:
            raise TypeError("conv4x4_winograd: x and dy of a weight gradient must have the same dtype")
    else:
        b = _req(b, torch.float32, "weight")
    res_dtype = torch.float32 if mode == 2 else (out_dtype or a.dtype)
    Ho, Wo = (H // 2, W // 2) if geom == GEOM_K4_S2_P3_D2 else (H - 1, W - 1)
    xs, ys, wsh = (B, Cin, H, W), (B, Cout, Ho, Wo), (Cout, Cin, 4, 4)
    want = {0: (xs, wsh, ys), 1: (ys, wsh, xs), 2: (xs, ys, wsh)}[mode]
    if tuple(a.shape) != want[0] or tuple(b.shape) != want[1]:
        raise RuntimeError("conv4x4_winograd mode %d: operands %s / %s do not match %s / %s" % (mode, tuple(a.shape), tuple(b.shape), want[0], want[1]))
    out = _result(out, want[2], res_dtype, a.device, "conv4x4_winograd")
    L = _lib.lib()
    ws = _probed_workspace(L, L.ipsr_conv4x4_winograd_workspace_bytes(geom, mode, B, Cin, H, W, Cout), a.device,
                           "ipsr_conv4x4_winograd: geometry %d mode %d Cin=%d Cout=%d %dx%d", (geom, mode, Cin, Cout, H, W))
    _lib.check(L.ipsr_conv4x4_winograd_mp(geom, mode, a.data_ptr(), b.data_ptr(), out.data_ptr(), B, Cin, H, W, Cout, MATH_CODE[math],
                                          _io_code(a_bf, res_dtype), ws.data_ptr(), ws.numel(), _stream()), "ipsr_conv4x4_winograd_mp")
    return out


S2_FINE_TO_COARSE, S2_COARSE_TO_FINE, S2_WEIGHT_GRAD = 0, 1, 2
S2_DILATED = 4          # or-ed into a data mode of conv4x4s2_bf16x3: pad 3, dilation 2 instead of pad 1
_S2_MODES = (S2_FINE_TO_COARSE, S2_COARSE_TO_FINE)
_S2_X3_MODES = _S2_MODES + (S2_DILATED | S2_FINE_TO_COARSE, S2_DILATED | S2_COARSE_TO_FINE)


def s2_winograd_supported(mode, B, Kc, Cf, nh, nw):
    return _lib.lib().ipsr_conv4x4s2_winograd_workspace_bytes(mode, B, Kc, Cf, nh, nw) > 0


def conv4x4s2_winograd(mode, a, b, B, Kc, Cf, nh, nw, out=None, math=None, out_dtype=None):
    """The k4 stride-2 pad-1 layers by Winograd F(5x5,2x2) on the polyphase components (ipsr_conv4x4s2_winograd_mp).
    fine = [B,Cf,2nh,2nw] (x of Conv2d, y of ConvTranspose2d), coarse = [B,Kc,nh,nw], weight = [Kc,Cf,4,4].
    mode 0 fine -> coarse (a = fine, b = weight), 1 coarse -> fine (a = coarse, b = weight), 2 weight gradient (a = fine, b = coarse;
    result fp32).  Activations fp32 or bf16; math: see MATH_CODE."""
    a, a_bf = _act(a, "operand a")
    if mode == 2:
        b, b_bf = _act(b, "operand b")
        if b_bf != a_bf:
            raise TypeError("conv4x4s2_winograd: both operands of a weight gradient must have the same dtype")
    else:
        b = _req(b, torch.float32, "weight")
    res_dtype = torch.float32 if mode == 2 else (out_dtype or a.dtype)
    fine, coarse, wsh = (B, Cf, 2 * nh, 2 * nw), (B, Kc, nh, nw), (Kc, Cf, 4, 4)
    want = {0: (fine, wsh, coarse), 1: (coarse, wsh, fine), 2: (fine, coarse, wsh)}[mode]
    if tuple(a.shape) != want[0] or tuple(b.shape) != want[1]:
        raise RuntimeError("conv4x4s2_winograd mode %d: operands %s / %s do not match %s / %s" % (mode, tuple(a.shape), tuple(b.shape), want[0], want[1]))
    out = _result(out, want[2], res_dtype, a.device, "conv4x4s2_winograd")
    L = _lib.lib()
    ws = _probed_workspace(L, L.ipsr_conv4x4s2_winograd_workspace_bytes(mode, B, Kc, Cf, nh, nw), a.device,
                           "ipsr_conv4x4s2_winograd: mode %d Kc=%d Cf=%d %dx%d", (mode, Kc, Cf, nh, nw))
    _lib.check(L.ipsr_conv4x4s2_winograd_mp(mode, a.data_ptr(), b.data_ptr(), out.data_ptr(), B, Kc, Cf, nh, nw, MATH_CODE[math],
                                            _io_code(a_bf, res_dtype), ws.data_ptr(), ws.numel(), _stream()), "ipsr_conv4x4s2_winograd_mp")
    return out


def thin_supported(op, Cin, H, W, Cout):
    """3x3 stride-1 pad-1 with 3 or 6 channels on one side (ipsr_conv3x3_thin): which side is thin depends on the operation."""
    fwd = op in (CONV_FWD, CONVT_FWD)
    i, o = (Cin, Cout) if fwd else (Cout, Cin)
    if i in (3, 6) and o % 16 == 0 and o >= 16:
        return W % 2 == 0
    return o in (3, 6) and W % 4 == 0 and i * o * 36 <= 48 * 1024 and i >= 16


def conv_to_one_supported(B, Cin, H, W, k, stride, pad, dil):
    """nn.Conv2d(Cin, 1, k, 1, pad) as ipsr_conv_to_one takes it (csrc/thin_conv.hip): a workspace probe, no kernel is launched."""
    if stride != 1 or dil != 1 or pad < 0 or k not in (3, 4):
        return False
    return _lib.lib().ipsr_conv_to_one_workspace_bytes(B, Cin, H, W, k, pad) > 0 and (2 * (H + 2 * pad) * (W + 2 * pad) + 2 * H * W + 64) * 4 <= 64 * 1024


def conv_to_one(x, w, pad):
    """y = conv2d(x, w, stride 1, padding pad) for w [1,C,K,K]: one pass over x (netD's last layer)."""
    x = _req(x, torch.float32, "input")
    w = _req(w, torch.float32, "weight")
    B, C, H, W = x.shape
    K = int(w.shape[-1])
    if tuple(w.shape) != (1, C, K, K):
        raise RuntimeError("conv_to_one: weight %s does not match %d input channels / one output" % (tuple(w.shape), C))
    y = _empty((B, 1, H + 2 * pad - K + 1, W + 2 * pad - K + 1), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    ws = _workspace(L.ipsr_conv_to_one_workspace_bytes(B, C, H, W, K, int(pad)), x.device)
    _lib.check(L.ipsr_conv_to_one(0, x.data_ptr(), w.data_ptr(), y.data_ptr(), B, C, H, W, K, int(pad), ws.data_ptr(), ws.numel(), _stream()),
               "ipsr_conv_to_one")
    return y


def conv_to_one_wrw(x, dy, K, pad, out=None):
    """dW [1,C,K,K] of the same layer: one pass over x."""
    x = _req(x, torch.float32, "input")
    dy = _req(dy, torch.float32, "grad_output")
    B, C, H, W = x.shape
    if tuple(dy.shape) != (B, 1, H + 2 * pad - K + 1, W + 2 * pad - K + 1):
        raise RuntimeError("conv_to_one_wrw: grad_output %s does not match input %s, k=%d, pad=%d" % (tuple(dy.shape), tuple(x.shape), K, pad))
    dw = _result(out, (1, C, K, K), torch.float32, x.device, "conv_to_one_wrw")
    _lib.check(_lib.lib().ipsr_conv_to_one(2, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, C, H, W, K, int(pad), None, 0, _stream()),
               "ipsr_conv_to_one")
    return dw


def conv3x3_thin(op, inp, weight, in_shape, Cout, bias=None, relu=False, out=None, out_dtype=None):
    """k3 s1 p1 Conv2d / ConvTranspose2d forward or backward-data with a 3- or 6-channel side (ipsr_conv3x3_thin_io).  `in_shape` =
    the module's input (B, Cin, H, W); `inp` is x for the forward ops and dy for the backward-data ops; bias / ReLU only few -> many.
    fp32 or bf16 activation tensors on either side (`out_dtype`, default = the input's); with a bf16 side the arithmetic is autocast's
    (bf16 operands, fp32 accumulation)."""
    B, Cin, H, W = in_shape
    inp, _ = _act(inp, "input")
    weight = _req(weight, torch.float32, "weight")
    out_dtype = out_dtype or (out.dtype if out is not None else inp.dtype)
    want_in, want_w, oshape = _data_pass_shapes(op, in_shape, Cout, 3, (H, W))
    I, O = want_in[1], oshape[1]
    if tuple(inp.shape) != want_in:
        raise RuntimeError("conv3x3_thin: input %s does not match %s" % (tuple(inp.shape), want_in))
    if tuple(weight.shape) != want_w:
        raise RuntimeError("conv3x3_thin op %d: weight %s does not match %s" % (op, tuple(weight.shape), want_w))
    if not thin_supported(op, Cin, H, W, Cout):
        raise NotImplementedError("conv3x3_thin op %d: Cin=%d Cout=%d %dx%d is not a thin-layer shape" % (op, Cin, Cout, H, W))
    so, si, flip = {CONV_FWD: (Cin * 9, 9, 0), CONV_BWD_DATA: (9, Cin * 9, 1), CONVT_FWD: (9, Cout * 9, 1), CONVT_BWD_DATA: (Cout * 9, 9, 0)}[op]
    io = _io_code(inp.dtype == torch.bfloat16, out_dtype)
    out = _result(out, oshape, out_dtype, inp.device, "conv3x3_thin")
    few2many = I in (3, 6) and O % 16 == 0
    _lib.check(_lib.lib().ipsr_conv3x3_thin_io(0 if few2many else 1, inp.data_ptr(), weight.data_ptr(), _ptr(_f32(bias)) if bias is not None else None,
                                               int(bool(relu)), out.data_ptr(), B, I, O, H, W, so, si, flip, io, _stream()), "ipsr_conv3x3_thin_io")
    return out


def conv3x3_thin_wrw(transposed, x, dy, out=None):
    """Weight gradient (fp32) of a k3 s1 p1 Conv2d ([Cout,Cin,3,3]) / ConvTranspose2d ([Cin,Cout,3,3]) with a 3- or 6-channel side; x and dy
    each fp32 or bf16."""
    x, _ = _act(x, "x")
    dy, _ = _act(dy, "dy")
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    wshape = (Cin, Cout, 3, 3) if transposed else (Cout, Cin, 3, 3)
    big, small = (x, dy) if transposed else (dy, x)            # G[big ch][small ch] is the weight's own [dim0][dim1] only when dim0 is wide
    Cb, Cs = big.shape[1], small.shape[1]
    L = _lib.lib()
    if Cs in (3, 6):
        g = _result(out, wshape, torch.float32, x.device, "conv3x3_thin_wrw")
        ws = _probed_workspace(L, L.ipsr_conv3x3_thin_wrw_workspace_bytes(B, Cb, Cs, H, W), x.device, "ipsr_conv3x3_thin_wrw: Cb=%d Cs=%d %dx%d", (Cb, Cs, H, W))
        io = int(big.dtype == torch.bfloat16) | (2 if small.dtype == torch.bfloat16 else 0)
        _lib.check(L.ipsr_conv3x3_thin_wrw_io(big.data_ptr(), small.data_ptr(), g.data_ptr(), B, Cb, Cs, H, W, io, ws.data_ptr(), ws.numel(), _stream()),
                   "ipsr_conv3x3_thin_wrw_io")
        return g
    raise NotImplementedError("conv3x3_thin_wrw: the weight's first channel dimension must be the wide one (got %s)" % (wshape,))


def _thin_f2m_geometry(op, B, Cin, H, W, Cout, k, stride):
    """(Cs, O, Ho, Wo, so, si, flip) of a few -> many pass in the terms of ipsr_conv_thin_f2m_mfma, or None: Conv2d forward (narrow input
    -> wide output on the strided grid) and ConvTranspose2d input gradient (narrow dy on the fine grid -> wide dx on the coarse one)."""
    T = k * k
    if op == CONV_FWD:
        if H % stride or W % stride:
            return None
        return Cin, Cout, H // stride, W // stride, Cin * T, T, 0
    if op == CONVT_BWD_DATA:                                   # dx[ci][iy][ix] = sum_{co,t} W[ci][co][t] dy[co][iy*st + r - pad][ix*st + s - pad]
        return Cout, Cin, H, W, Cout * T, T, 0
    return None


def thin_f2m_mfma_supported(op, B, Cin, H, W, Cout, k, stride):
    g = _thin_f2m_geometry(op, B, Cin, H, W, Cout, k, stride)
    return g is not None and bool(_lib.lib().ipsr_conv_thin_f2m_mfma_supported(B, g[0], g[1], g[2], g[3], k, stride))


def conv_thin_f2m_mfma(op, inp, weight, in_shape, Cout, k, stride, bias=None, relu=False, out_dtype=torch.bfloat16):
    """Conv2d forward / ConvTranspose2d input gradient with 3 or 6 channels on the narrow (read) side on the bf16 matrix cores
    (ipsr_conv_thin_f2m_mfma): k3 s1 p1 or k4 s2 p1.  `in_shape` = the module's input (B, Cin, H, W); `inp` = x (forward) or dy (input
    gradient), fp32 or bf16 (rounded to bf16 inside); bias / ReLU in fp32; bf16 or fp32 out."""
    B, Cin, H, W = in_shape
    inp, in_bf = _act(inp, "input")
    weight = _req(weight, torch.float32, "weight")
    g = _thin_f2m_geometry(op, B, Cin, H, W, Cout, k, stride)
    if g is None or not _lib.lib().ipsr_conv_thin_f2m_mfma_supported(B, g[0], g[1], g[2], g[3], k, stride):
        raise NotImplementedError("conv_thin_f2m_mfma op %d: Cin=%d Cout=%d %dx%d k%d s%d is not implemented" % (op, Cin, Cout, H, W, k, stride))
    Cs, O, Ho, Wo, so, si, flip = g
    want_in = (B, Cs, Ho * stride, Wo * stride)
    want_w = (Cout, Cin, k, k) if op == CONV_FWD else (Cin, Cout, k, k)
    if tuple(inp.shape) != want_in or tuple(weight.shape) != want_w:
        raise RuntimeError("conv_thin_f2m_mfma op %d: input %s / weight %s do not match %s / %s" % (op, tuple(inp.shape), tuple(weight.shape), want_in, want_w))
    out = _empty((B, O, Ho, Wo), dtype=out_dtype, device=inp.device)
    _lib.check(_lib.lib().ipsr_conv_thin_f2m_mfma(inp.data_ptr(), weight.data_ptr(), _ptr(_f32(bias)) if bias is not None else None, int(bool(relu)),
                                                  out.data_ptr(), B, Cs, O, Ho, Wo, k, stride, so, si, flip, _io_code(in_bf, out_dtype), _stream()),
               "ipsr_conv_thin_f2m_mfma")
    return out


def thin_wrw_mfma_supported(transposed, B, Cin, H, W, Cout, k, stride):
    """Weight gradient of a k3 s1 p1 / k4 s2 p1 layer with 3 or 6 channels on its NARROW side on the bf16 matrix cores: the wide side
    must be the weight's first dimension (Conv2d: Cout wide; ConvTranspose2d: Cin wide) and live on the coarse grid."""
    if transposed:
        Kb, Cs, Hb, Wb = Cin, Cout, H, W                   # big = x on the module's input grid (the coarse one)
    else:
        if H % stride or W % stride:
            return False
        Kb, Cs, Hb, Wb = Cout, Cin, H // stride, W // stride
    return _lib.lib().ipsr_conv_thin_wrw_mfma_workspace_bytes(B, Kb, Cs, Hb, Wb, k, stride) > 0


def conv_thin_wrw_mfma(transposed, x, dy, k, stride, out=None):
    """-> dW (fp32, the module's layout) of a thin Conv2d / ConvTranspose2d on the matrix cores (ipsr_conv_thin_wrw_mfma).  A bf16 wide
    tensor multiplies in bf16 (the narrow one may be fp32: it is rounded inside, as autocast's cast would); fp32 tensors multiply in fp32."""
    x, _ = _act(x, "x")
    dy, _ = _act(dy, "dy")
    big, small = (x, dy) if transposed else (dy, x)
    if big.dtype == torch.float32 and small.dtype != torch.float32:
        raise TypeError("conv_thin_wrw_mfma: an fp32 wide tensor needs an fp32 narrow one")
    B, Kb, Hb, Wb = big.shape
    Cs = small.shape[1]
    if tuple(small.shape) != (B, Cs, Hb * stride, Wb * stride):
        raise RuntimeError("conv_thin_wrw_mfma: narrow tensor %s does not match wide %s at stride %d" % (tuple(small.shape), tuple(big.shape), stride))
    L = _lib.lib()
    g = _result(out, (Kb, Cs, k, k), torch.float32, x.device, "conv_thin_wrw_mfma")
    ws = _probed_workspace(L, L.ipsr_conv_thin_wrw_mfma_workspace_bytes(B, Kb, Cs, Hb, Wb, k, stride), x.device,
                           "ipsr_conv_thin_wrw_mfma: Kb=%d Cs=%d %dx%d k%d s%d", (Kb, Cs, Hb, Wb, k, stride))
    _lib.check(L.ipsr_conv_thin_wrw_mfma(big.data_ptr(), small.data_ptr(), g.data_ptr(), B, Kb, Cs, Hb, Wb, k, stride, int(big.dtype == torch.bfloat16) | (2 if small.dtype == torch.bfloat16 else 0),
                                         ws.data_ptr(), ws.numel(), _stream()), "ipsr_conv_thin_wrw_mfma")
    return g


SM_DATA, SM_WRW, SM_FWD = 0, 1, 2


SM_TILED = 16           # flag bit of `op` (IPSR_SMALLMAP_TILED): the LDS-tiled GEMMs for SM_DATA / SM_FWD above 32 positions


def smallmap_supported(op, B, R, Cq, Ho, Wo, Hf, Wf, k, stride, pad, dil, tiled=False):
    return _lib.lib().ipsr_conv_smallmap_workspace_bytes(op | (SM_TILED if tiled else 0), B, R, Cq, Ho, Wo, Hf, Wf, k, stride, pad, dil) > 0


def conv_smallmap(op, a, b, B, R, Cq, Ho, Wo, Hf, Wf, k, stride, pad, dil, out=None, tiled=False):
    """Small-map convolutions with the weight tensor [R,Cq,k,k] as the GEMM operand in place (ipsr_conv_smallmap):
    op SM_DATA: a = in [B,R,Ho,Wo], b = weight -> [B,Cq,Hf,Wf] (Conv2d backward-data / ConvTranspose2d forward);
    op SM_WRW:  a = coarse [B,R,Ho,Wo], b = fine [B,Cq,Hf,Wf] -> dW [R,Cq,k,k];
    op SM_FWD:  a = fine [B,Cq,Hf,Wf], b = weight -> [B,R,Ho,Wo] (Conv2d forward / ConvTranspose2d backward-data).
    tiled: the call carries SM_TILED (the regime for 33 .. 1024 positions; the weight gradient has none and runs as without it)."""
    a = _req(a, torch.float32, "operand a")
    b = _req(b, torch.float32, "operand b")
    coarse, fine, wsh = (B, R, Ho, Wo), (B, Cq, Hf, Wf), (R, Cq, k, k)
    want = {SM_DATA: (coarse, wsh, fine), SM_WRW: (coarse, fine, wsh), SM_FWD: (fine, wsh, coarse)}[op]
    if tuple(a.shape) != want[0] or tuple(b.shape) != want[1]:
        raise RuntimeError("conv_smallmap op %d: operands %s / %s do not match %s / %s" % (op, tuple(a.shape), tuple(b.shape), want[0], want[1]))
    out = _result(out, want[2], torch.float32, a.device, "conv_smallmap")
    L = _lib.lib()
    op |= SM_TILED if tiled else 0
    ws = _probed_workspace(L, L.ipsr_conv_smallmap_workspace_bytes(op, B, R, Cq, Ho, Wo, Hf, Wf, k, stride, pad, dil), a.device,
                           "ipsr_conv_smallmap: op %d R=%d Cq=%d %dx%d -> %dx%d k%d s%d p%d d%d", (op, R, Cq, Hf, Wf, Ho, Wo, k, stride, pad, dil))
    _lib.check(L.ipsr_conv_smallmap(op, a.data_ptr(), b.data_ptr(), out.data_ptr(), B, R, Cq, Ho, Wo, Hf, Wf, k, stride, pad, dil,
                                    ws.data_ptr(), ws.numel(), _stream()), "ipsr_conv_smallmap")
    return out


def conv3x3_winograd_wrw(transposed, x, dy, Cout, out=None, math=None):
    """Weight gradient of a k3 s1 p1 Conv2d (transposed=False -> [Cout,Cin,3,3]) / ConvTranspose2d (True -> [Cin,Cout,3,3]).
    out: optional contiguous fp32 tensor of that shape to write into (e.g. a slice of a gradient bucket).  x / dy fp32 or bf16 (both
    the same); the result is fp32; math: see MATH_CODE."""
    x, x_bf = _act(x, "conv input")
    dy, dy_bf = _act(dy, "grad_output")
    if x_bf != dy_bf:
        raise TypeError("conv3x3_winograd_wrw: x and dy must have the same dtype")
    B, Cin, H, W = x.shape
    if tuple(dy.shape) != (B, Cout, H, W):
        raise RuntimeError("conv3x3_winograd_wrw: grad_output %s does not match %s" % (tuple(dy.shape), (B, Cout, H, W)))
    dw = _result(out, (Cin, Cout, 3, 3) if transposed else (Cout, Cin, 3, 3), torch.float32, x.device, "conv3x3_winograd_wrw")
    L = _lib.lib()
    ws = _workspace(L.ipsr_conv3x3_winograd_wrw_workspace_bytes(int(transposed), B, Cin, H, W, Cout), x.device)
    _lib.check(L.ipsr_conv3x3_winograd_wrw_mp(int(transposed), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, Cin, H, W, Cout, MATH_CODE[math],
                                              int(x_bf), ws.data_ptr(), ws.numel(), _stream()), "ipsr_conv3x3_winograd_wrw_mp")
    return dw


_IC_TICKETS = {}


def innercos_loss(x, cuse, mask_f32, target, strength, one_launch=False):
    """K9.  x [B,Cx,h,w] (only the first `cuse` channels are read), target [B,cuse,h,w] -> loss [] fp32.
    mask_f32: N = h*w elements (one mask for the batch), or B*N ([B,h,w]: one mask per sample, the `_masks` entry)."""
    x = _req(x, torch.float32, "in_data")
    target = _req(target, torch.float32, "target")
    mask = _req(mask_f32, torch.float32, "mask")
    B, Cx = x.shape[0], x.shape[1]
    N = x.shape[2] * x.shape[3]
    per_sample = B > 1 and mask.numel() == B * N
    if tuple(target.shape) != (B, cuse, x.shape[2], x.shape[3]) or not (mask.numel() == N or per_sample):
        raise RuntimeError("InnerCos: target %s / mask %s do not match input %s" % (tuple(target.shape), tuple(mask.shape), tuple(x.shape)))
    if per_sample and one_launch:
        raise RuntimeError("InnerCos: the one-launch form takes one mask for the batch")
    loss = _empty((), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    ws = _workspace(L.innercos_workspace_bytes(B, cuse, N), x.device)
    if per_sample:
        _lib.check(L.innercos_loss_masks(x.data_ptr(), B, Cx, cuse, N, mask.data_ptr(), N, target.data_ptr(), float(strength),
                                         loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "innercos_loss_masks")
    elif one_launch:
        _lib.check(L.innercos_loss_fused(x.data_ptr(), B, Cx, cuse, N, mask.data_ptr(), target.data_ptr(), float(strength),
                                         loss.data_ptr(), ws.data_ptr(), ws.numel(), _innercos_ticket(x.device).data_ptr(), _stream()),
                   "innercos_loss_fused")
    else:
        _lib.check(L.innercos_loss(x.data_ptr(), B, Cx, cuse, N, mask.data_ptr(), target.data_ptr(), float(strength),
                                   loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "innercos_loss")
    return loss


def _innercos_ticket(device):
    """The arrival counter of the one-launch form, whose last workgroup folds the block partials: a word of OUR memory, one per (device,
    stream) — the calls of a stream are ordered, and every launch leaves the word zero — allocated (zeroed) once.  The form is measured
    SLOWER than two launches (csrc/innercos.hip): kept for the C-ABI's completeness and its test, not used by the modules."""
    key = (device.index, _stream())
    ticket = _IC_TICKETS.get(key)
    if ticket is None:
        ticket = _IC_TICKETS[key] = _zeros(64, dtype=torch.int32, device=device)
    return ticket


def innercos_loss_backward(x, cuse, mask_f32, target, strength, grad_loss):
    x = _req(x, torch.float32, "in_data")
    target = _req(target, torch.float32, "target")
    mask = _req(mask_f32, torch.float32, "mask")
    gl = _req(grad_loss.reshape(1).to(torch.float32), torch.float32, "grad_loss")
    B, Cx = x.shape[0], x.shape[1]
    N = x.shape[2] * x.shape[3]
    per_sample = B > 1 and mask.numel() == B * N
    if not (mask.numel() == N or per_sample):
        raise RuntimeError("InnerCos: mask %s does not match input %s" % (tuple(mask.shape), tuple(x.shape)))
    gx = _empty(x.shape, x.dtype, x.device)
    if per_sample:
        _lib.check(_lib.lib().innercos_loss_backward_masks(x.data_ptr(), B, Cx, cuse, N, mask.data_ptr(), N, target.data_ptr(),
                                                           float(strength), gl.data_ptr(), gx.data_ptr(), _stream()),
                   "innercos_loss_backward_masks")
    else:
        _lib.check(_lib.lib().innercos_loss_backward(x.data_ptr(), B, Cx, cuse, N, mask.data_ptr(), target.data_ptr(),
                                                     float(strength), gl.data_ptr(), gx.data_ptr(), _stream()),
                   "innercos_loss_backward")
    return gx


# ---- loss heads (csrc/loss_head.hip): the value and the gradients for a unit incoming gradient in one launch
def _count(n, what):
    if not 0 < n < 2 ** 31:
        raise RuntimeError("%s: %d elements (the entry takes 1 .. 2^31 - 1)" % (what, n))
    return n


def ragan_loss(fake, real, s, want_fake=True, want_real=True, joined=False):
    """The relativistic-average LSGAN loss 1/2 [mean((real - mean(fake) - s)^2) + mean((fake - mean(real) + s)^2)] of two fp32
    predictions (any shapes, the sizes may differ) -> (loss [], d loss / d fake or None, d loss / d real or None), the gradients shaped
    like their inputs.  `joined`: both gradients are wanted as ONE flat buffer [n_fake + n_real] (fake first) -> (loss, buffer): the
    gradient of a batched prediction whose halves `fake` and `real` are."""
    fake, real = _req(fake, torch.float32, "fake"), _req(real, torch.float32, "real")
    nf, nr = _count(fake.numel(), "fake"), _count(real.numel(), "real")
    _count(nf + nr, "fake + real")
    dev = fake.device
    loss = _empty((), dtype=torch.float32, device=dev)
    if joined:
        both = _empty((nf + nr,), dtype=torch.float32, device=dev)
        gf, gr = both[:nf], both[nf:]
    else:
        gf = _empty(fake.shape, dtype=torch.float32, device=dev) if want_fake else None
        gr = _empty(real.shape, dtype=torch.float32, device=dev) if want_real else None
    _lib.check(_lib.lib().ipsr_ragan_loss(fake.data_ptr(), nf, real.data_ptr(), nr, float(s), loss.data_ptr(),
                                          gf.data_ptr() if gf is not None else None, gr.data_ptr() if gr is not None else None, _stream()),
               "ipsr_ragan_loss")
    return (loss, both) if joined else (loss, gf, gr)


def l1_pair_loss(a1, a2, target, scale, want1=True, want2=True):
    """scale * (mean|a1 - target| + mean|a2 - target|) of three fp32 tensors of one shape -> (loss [], g1 or None, g2 or None) with
    g = (scale / n) * sign(a - target), written in the same pass."""
    a1, a2, target = _req(a1, torch.float32, "a1"), _req(a2, torch.float32, "a2"), _req(target, torch.float32, "target")
    if a1.shape != target.shape or a2.shape != target.shape:
        raise RuntimeError("l1_pair_loss: shapes %s / %s / %s differ" % (tuple(a1.shape), tuple(a2.shape), tuple(target.shape)))
    n, dev = _count(target.numel(), "target"), target.device
    loss = _empty((), dtype=torch.float32, device=dev)
    g1 = _empty(a1.shape, dtype=torch.float32, device=dev) if want1 else None
    g2 = _empty(a2.shape, dtype=torch.float32, device=dev) if want2 else None
    L = _lib.lib()
    ws = _workspace(L.ipsr_l1_pair_loss_workspace_bytes(n), dev)
    _lib.check(L.ipsr_l1_pair_loss(a1.data_ptr(), a2.data_ptr(), target.data_ptr(), n, float(scale), loss.data_ptr(),
                                   g1.data_ptr() if g1 is not None else None, g2.data_ptr() if g2 is not None else None,
                                   ws.data_ptr(), ws.numel(), _stream()), "ipsr_l1_pair_loss")
    return loss, g1, g2


def loss_grad_scale(grad_loss, g1, g2=None):
    """The backward of the loss heads: g * grad_loss for one or two saved gradients in one launch; grad_loss is a one-element fp32
    tensor on the device and stays there."""
    gl = _req(grad_loss.reshape(1), torch.float32, "grad_loss")
    g1 = _req(g1, torch.float32, "g1")
    _count(g1.numel(), "g1")
    o1 = _empty(g1.shape, dtype=torch.float32, device=g1.device)
    o2 = None
    if g2 is not None:
        g2 = _req(g2, torch.float32, "g2")
        _count(g2.numel(), "g2")
        o2 = _empty(g2.shape, dtype=torch.float32, device=g2.device)
    _lib.check(_lib.lib().ipsr_loss_grad_scale(gl.data_ptr(), g1.data_ptr(), o1.data_ptr(), g1.numel(),
                                               g2.data_ptr() if g2 is not None else None, o2.data_ptr() if o2 is not None else None,
                                               g2.numel() if g2 is not None else 0, _stream()), "ipsr_loss_grad_scale")
    return o1, o2


# ---- image quality (csrc/image_quality.hip): per-image SSIM, mean (x - y)^2 and mean |x - y| of a batch
IQ_SSIM = 1                     # IPSR_IQ_SSIM of include/ipsr_hip.h
_iq_windows = {}


def ssim_window():
    """The 11x11 SSIM window of DESIGN.md "Image quality": Gaussian of sigma 1.5 over mgrid[-5:6, -5:6], normalised, rounded to
    float32 -> numpy float32 [11,11]."""
    import numpy as np
    x, y = np.mgrid[-5:6, -5:6]
    g = np.exp(-(x ** 2 + y ** 2) / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(np.float32)


def _iq_window(device):
    """The window widened to float64 on `device` (121 doubles, made once per device)."""
    w = _iq_windows.get(device.index)
    if w is None:
        w = torch.from_numpy(ssim_window().astype("float64").reshape(-1)).to(device)
        _iq_windows[device.index] = w
    return w


def image_quality(x, y, ssim=True):
    """x, y [B,C,H,W] (fp32; bf16 / fp16 are taken with .float()) -> float64 [B,3] on the device: per image the mean SSIM map, the
    mean (x - y)^2 and the mean |x - y|.  ssim=False: column 0 is NaN (not computed), columns 1-2 are the same bits, any H, W >= 1.
    No host synchronisation; runs on the current stream."""
    if torch.is_tensor(x) and x.dtype in (torch.bfloat16, torch.float16):
        x = x.float()
    if torch.is_tensor(y) and y.dtype in (torch.bfloat16, torch.float16):
        y = y.float()
    x, y = _req(x, torch.float32, "x"), _req(y, torch.float32, "y")
    if x.dim() != 4 or x.shape != y.shape:
        raise RuntimeError("image_quality: x %s and y %s must be two [B,C,H,W] tensors of one shape" % (tuple(x.shape), tuple(y.shape)))
    B, C, H, W = x.shape
    flags = IQ_SSIM if ssim else 0
    L = _lib.lib()
    nbytes = L.ipsr_image_quality_workspace_bytes(B, C, H, W, flags)
    if nbytes == 0:                                     # refused shape: the entry itself says why, before any launch
        _lib.check(L.ipsr_image_quality(x.data_ptr(), y.data_ptr(), B, C, H, W, flags, None, None, None, 0, _stream()), "ipsr_image_quality")
    win = _iq_window(x.device) if ssim else None
    out = _empty((B, 3), dtype=torch.float64, device=x.device)
    ws = _workspace(nbytes, x.device)
    _lib.check(L.ipsr_image_quality(x.data_ptr(), y.data_ptr(), B, C, H, W, flags, win.data_ptr() if ssim else None, out.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream()), "ipsr_image_quality")
    return out
