"""Thin torch<->C-ABI marshalling: tensors in, tensors out, raw device pointers underneath.
PyTorch is used for device memory and streams only; every op here runs a kernel of libegomi.so.
"""
import ctypes
import math

import torch

from . import _abi, _lib
from ._lib import c_p, c_i, c_d, c_f, c_sz, c_i64, call, query  # noqa: F401  (the c_* names: tests and tools build arguments with them)

F32, BF16 = _abi.EGOMI_F32, _abi.EGOMI_BF16


def dt(t: torch.dtype) -> int:
    if t == torch.float32:
        return F32
    if t == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t}")


def P(t):
    if t is None:
        return c_p(None)
    if not t.is_cuda:
        raise _lib.EgomiError("egoscaler_amd ops need CUDA/HIP tensors (no CPU fallback)")
    return c_p(t.data_ptr())


def S():
    return c_p(torch.cuda.current_stream().cuda_stream)


def _c(t, dtype=None):
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------ A1/A2
def unproject_gather(rgb, depth, pp, fx, fy, d_thres=None, boxes=None, n_out=0):
    """rgb u8 [B,T,H,W,3], depth f32 [B,T,H,W] -> (points f64 [B,cap,3], colors f32 [B,cap,3],
    count i32 [B]).  See include/egomi.h (A1)."""
    rgb, depth = _c(rgb, torch.uint8), _c(depth, torch.float32)
    B, T, H, W, _ = rgb.shape
    cap = n_out if n_out > 0 else T * H * W
    dev = rgb.device
    pts = torch.empty(B, cap, 3, dtype=torch.float64, device=dev)
    col = torch.empty(B, cap, 3, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    ws_bytes = query("egomi_unproject_workspace_bytes", B, T, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    bx, nb = None, 0
    if boxes is not None and len(boxes):
        bx = torch.tensor([[b["ymin"], b["ymax"], b["xmin"], b["xmax"]] for b in boxes], dtype=torch.int32, device=dev)
        nb = bx.shape[0]
    call("egomi_unproject_gather", rgb, depth, bx, nb, B, T, H, W, pp, fx, fy, float("nan") if d_thres is None else d_thres, n_out, pts, col, cnt, ws,
         ws_bytes, S())
    return pts, col, cnt


def depth_to_cloud(pred, rgb, final_width, final_height, focal_len_x=0, focal_len_y=0, principal_point=0):
    """N4 (depth.py:35-62): pred f32 [B,h0,w0] or [h0,w0], rgb u8 [B,H,W,3] or [H,W,3] ->
    (z f32 [.., H, W], points f64 [.., H*W, 3] | None, colors f64 [.., H*W, 3] | None)."""
    single = pred.dim() == 2
    pred = _c(pred if not single else pred[None], torch.float32)
    B, h0, w0 = pred.shape
    H, W = int(final_height), int(final_width)
    dev = pred.device
    want = focal_len_x > 0 and focal_len_y > 0 and principal_point > 0            # depth.py:53
    z = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    tab = torch.empty(W + H, dtype=torch.int32, device=dev)
    pts = col = None
    if want:
        rgb = _c(rgb if rgb.dim() == 4 else rgb[None], torch.uint8)
        if tuple(rgb.shape) != (B, H, W, 3):
            raise ValueError(f"depth_to_cloud: rgb must be [{B},{H},{W},3], got {tuple(rgb.shape)}")
        pts = torch.empty(B, H * W, 3, dtype=torch.float64, device=dev)
        col = torch.empty(B, H * W, 3, dtype=torch.float64, device=dev)
    call("egomi_depth_to_cloud", pred, B, h0, w0, rgb if want else None, H, W, float(focal_len_x), float(focal_len_y), float(principal_point), tab, z,
         pts, col, S())
    if single:
        return z[0], (pts[0] if want else None), (col[0] if want else None)
    return z, pts, col


def pc_norm(points, colors):
    points, colors = _c(points, torch.float64), _c(colors, torch.float32)
    B, N, _ = points.shape
    out = torch.empty(B, N, 6, dtype=torch.float32, device=points.device)
    call("egomi_pc_norm", points, colors, out, B, N, S())
    return out


# ------------------------------------------------------------------------------------------ A3-A5
def fps(pts, start, num_group):
    pts = _c(pts, torch.float32)
    B, N, C = pts.shape
    if torch.is_tensor(start) and start.is_cuda and start.dtype == torch.int32 and start.numel() == B:
        start = start.contiguous()          # resident start vector: validated by its producer (no host sync here)
    else:
        host = torch.as_tensor(start).reshape(-1).to(torch.int64).cpu()
        if host.numel() != B or int(host.min()) < 0 or int(host.max()) >= N:
            raise ValueError("fps: start must hold one index in [0,N) per cloud")
        start = host.to(torch.int32).to(pts.device)
    idx = torch.empty(B, num_group, dtype=torch.int32, device=pts.device)
    cen = torch.empty(B, num_group, 3, dtype=torch.float32, device=pts.device)
    call("egomi_fps", pts, B, N, C, start, num_group, idx, cen, S())
    return idx, cen


def knn_group(pts, center, k, out_dtype=torch.float32):
    pts, center = _c(pts, torch.float32), _c(center, torch.float32)
    B, N, C = pts.shape
    G = center.shape[1]
    idx = torch.empty(B, G, k, dtype=torch.int32, device=pts.device)
    nb = torch.empty(B, G, k, C, dtype=out_dtype, device=pts.device)
    call("egomi_knn_group", pts, center, B, N, C, G, k, idx, nb, dt(out_dtype), S())
    return idx, nb


# ------------------------------------------------------------------------------------------ GEMM
GemmDesc = _abi.STRUCTS["egomi_gemm_desc"]               # generated from the header's typedef, field for field

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2


class GemmProfiler:
    """HIP-event timing of GEMM launches on the stream they are launched on (bench.py roofline)."""

    def __init__(self, min_flops=1e9, tuned_only=True, kernel_ids=None):
        """kernel_ids: egomi_gemm_kernel_id() values to record (None: 1 and 2 when tuned_only, else everything)."""
        self.min_flops, self.recs, self.enabled, self.tuned_only = min_flops, [], True, tuned_only
        self.kernel_ids = kernel_ids if kernel_ids is not None else ((1, 2) if tuned_only else None)

    def summary(self):
        """launches / flops / ms: the recorded brackets.  For launches of the 256x256 kernel (kernel id 2) `ms` is that kernel alone
        (events recorded by the library around it: egomi_gemm_time_next) and `call_ms` the whole egomi_gemm call, i.e. including
        the slab-combine pass of K-sliced tail rows; for other kernels both are the call."""
        torch.cuda.synchronize()
        n, flops, ms, call_ms = 0, 0.0, 0.0, 0.0
        for e0, e1, f, k0, k1 in self.recs:
            n += 1
            flops += f
            c = e0.elapsed_time(e1)
            call_ms += c
            if k0 is not None:
                t = ctypes.c_float()
                ms += t.value if query("egomi_event_elapsed_ms", k0, k1, ctypes.byref(t)) == 0 else c     # never recorded (opt-in persistent form): the call
            else:
                ms += c
        return {"launches": n, "flops": flops, "ms": ms, "call_ms": call_ms}

    def __del__(self):
        try:
            for _, _, _, k0, k1 in self.recs:
                if k0 is not None:
                    query("egomi_event_destroy", k0)
                    query("egomi_event_destroy", k1)
        except Exception:
            pass


PROFILER = None


_TAIL_WS = {}


def _tail_workspace(device, nbytes=(4096 + 256 * 2 * 262144)):
    """One fp32 scratch buffer per device, shared by every large product (launches are stream-ordered): 4 KB of ticket words
    (zero here, returned to zero by every launch: include/egomi.h `ws_tickets_zeroed`) + the fp32 slabs of shared tiles."""
    ws = _TAIL_WS.get(device)
    if ws is None:
        ws = _TAIL_WS[device] = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
    return ws


def gemm_raw(A, B, C, M, N, K, lda, ldb, ldc, a_layout=0, b_layout=0, bias=None, residual=None, ldr=0,
             act=0, alpha=1.0, accumulate=False, batch=1, batch_inner=1, strides=(0, 0, 0, 0, 0, 0), force_generic=False,
             workspace=None, split_k=0, persistent=None, swiglu_out=None, slabs=False, count_only=False, defer_tail=False, swiglu_bwd_gu=None):
    """C = act(alpha*A.B + bias) + residual (+C).  A/B/C are tensors whose data_ptr() is the first
    element of the (first) operand; all strides in elements.  See include/egomi.h."""
    if A.dtype != B.dtype:
        raise TypeError("gemm: A and B dtypes differ")
    d = GemmDesc()
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), C.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    if bias is not None and bias.dtype != A.dtype:
        raise TypeError("gemm: bias dtype must equal the operand dtype")
    if residual is not None and residual.dtype != C.dtype:
        raise TypeError("gemm: residual dtype must equal the output dtype")
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.a_layout, d.b_layout = a_layout, b_layout
    d.ab_dtype, d.c_dtype = dt(A.dtype), dt(C.dtype)
    d.batch, d.batch_inner = batch, batch_inner
    d.sA0, d.sA1, d.sB0, d.sB1, d.sC0, d.sC1 = strides
    d.alpha, d.accumulate, d.act, d.force_generic = alpha, int(accumulate), act, int(force_generic)
    if swiglu_out is not None:                            # EGOMI_EPI_SWIGLU: C = interleaved-32 gate|up, swiglu_out [M, N/2] = silu(gate)*up
        d.epilogue, d.C2, d.ldc2 = _abi.EGOMI_EPI_SWIGLU, swiglu_out.data_ptr(), _ld(swiglu_out)
    if swiglu_bwd_gu is not None:                         # EGOMI_EPI_SWIGLU_BWD: the product is d(act); C = d(gate|up) [M, 2N], C2 = gate|up [M, 2N] (interleaved-32)
        if swiglu_out is not None or swiglu_bwd_gu.dtype != C.dtype:
            raise TypeError("gemm: swiglu_bwd_gu excludes swiglu_out and must have the output dtype")
        d.epilogue, d.C2, d.ldc2 = _abi.EGOMI_EPI_SWIGLU_BWD, swiglu_bwd_gu.data_ptr(), _ld(swiglu_bwd_gu)
    if workspace is None and M >= 1024 and batch <= 1:
        workspace = _tail_workspace(A.device)            # ticket words + fp32 slabs for the shared tiles of the 256x256 kernel
        if persistent is False:                          # A/B runs, tests: the non-persistent kernel + combine launch; its slabs must
            workspace = workspace[1024:]                 # stay clear of the ticket words the persistent launches rely on
        else:
            d.ws_tickets_zeroed = 2 if persistent else 1  # True: wherever the persistent form can run; None: the library's measured rule
    if workspace is not None:
        d.workspace, d.workspace_bytes, d.split_k = workspace.data_ptr(), workspace.numel() * workspace.element_size(), split_k
    for t in (A, B, C):
        if not t.is_cuda:
            raise _lib.EgomiError("gemm needs device tensors")
    if slabs or count_only:                               # EGOMI_EPI_SLABS: K-slice slabs stay unsummed in `workspace`; -> their number
        d.epilogue = _abi.EGOMI_EPI_SLABS
        n = query("egomi_gemm_slab_count", ctypes.byref(d))
        if count_only:
            return n
        if n < 2:
            raise _lib.EgomiError("gemm: the library would not split this product (egomi_gemm_slab_count == 0)")
        call("egomi_gemm", ctypes.byref(d), S())
        return n
    tail = None
    if defer_tail and d.workspace and bias is None and act == 0 and alpha == 1.0 and not accumulate and swiglu_out is None and \
            C.dtype == torch.bfloat16:
        # EGOMI_EPI_SLABS on a large product: the K-sliced tail rows stay as fp32 slabs for the caller's next kernel (ops.rmsnorm /
        # ops.rmsnorm_bwd with tail=...); nothing changes when the library's plan has no such rows for this shape
        row0, slices = c_i(0), c_i(0)
        if query("egomi_gemm_tail_plan", ctypes.byref(d), ctypes.byref(row0), ctypes.byref(slices)) == 0 and slices.value >= 2:
            d.epilogue = _abi.EGOMI_EPI_SLABS
            if query("egomi_gemm_kernel_id", ctypes.byref(d)) == 2:    # the launch must take the kernel the plan was made for
                tail = (row0.value, slices.value, d.workspace + (4096 if d.ws_tickets_zeroed else 0))
            else:
                d.epilogue = _abi.EGOMI_EPI_NONE
    prof = PROFILER
    flops = 2.0 * M * N * K * max(1, batch)
    kid = query("egomi_gemm_kernel_id", ctypes.byref(d)) if (prof is not None and prof.enabled and flops >= prof.min_flops) else None
    if kid is not None and (prof.kernel_ids is None or kid in prof.kernel_ids):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k0 = k1 = None
        if kid == 2:                                        # the 256x256 kernel: the library brackets the kernel itself
            k0, k1 = c_p(), c_p()
            call("egomi_event_create", ctypes.byref(k0))
            call("egomi_event_create", ctypes.byref(k1))
            call("egomi_gemm_time_next", k0, k1)
        e0.record()
        call("egomi_gemm", ctypes.byref(d), S())
        e1.record()
        prof.recs.append((e0, e1, flops, k0, k1))
    else:
        call("egomi_gemm", ctypes.byref(d), S())
    return (C, tail) if defer_tail else C


def _ld(t):
    if t.dim() != 2 or (t.shape[1] != 1 and t.stride(1) != 1):
        raise ValueError("expected a 2-D view with unit inner stride")
    return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]


def mm(a, b, out=None, a_layout=0, b_layout=0, out_dtype=None, **kw):
    """2-D product on views with unit inner stride.  a: [M,K] (layout 0) or [K,M] (1);
    b: [N,K] (layout 0, nn.Linear weight) or [K,N] (1)."""
    M, K = (a.shape if a_layout == 0 else (a.shape[1], a.shape[0]))
    N, Kb = (b.shape if b_layout == 0 else (b.shape[1], b.shape[0]))
    if K != Kb:
        raise ValueError(f"mm: inner dims differ ({K} vs {Kb})")
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype or a.dtype, device=a.device)
    res = kw.get("residual")
    return gemm_raw(a, b, out, M, N, K, _ld(a), _ld(b), _ld(out), a_layout, b_layout,
                    ldr=_ld(res) if res is not None else 0, **kw)


def mm_slabs(a, b, out_like, workspace, count_only=False):
    """a [M,K] . b[N,K]^T with M <= 512 as UNSUMMED fp32 K-slice slabs [slices, M, N] at the start of `workspace` (include/egomi.h,
    EGOMI_EPI_SLABS); returns the number of slices (count_only: without launching; 0 = the library would not split it).
    `out_like` [M,N] only lends its dtype / alignment to the descriptor, it is not written."""
    M, K = a.shape
    N = b.shape[0]
    return gemm_raw(a, b, out_like, M, N, K, _ld(a), _ld(b), _ld(out_like), workspace=workspace, slabs=not count_only, count_only=count_only)


def slabs_rmsnorm(workspace, slices, residual, w, eps, x_out, h_out):
    """x_out = round(sum of the slabs + residual), h_out = rmsnorm(x_out) * w  (egomi_slabs_rmsnorm)."""
    rows, cols = x_out.shape
    call("egomi_slabs_rmsnorm", workspace, slices, rows, cols, residual, _ld(residual) if residual is not None else 0, w, eps, x_out, _ld(x_out),
         h_out, _ld(h_out), dt(x_out.dtype), S())


def qkv_finish(workspace, slices, qkv, cos, sin, pos, kc, vc, B, H, hd, Smax):
    """q|k|v = round(sum of the slabs); RoPE(pos) on q and k; q -> qkv, k / v -> the caches at `pos`  (egomi_qkv_finish)."""
    call("egomi_qkv_finish", workspace, slices, qkv, _ld(qkv), cos, sin, pos, kc, vc, B, H, hd, Smax, dt(qkv.dtype), S())


def qkv_finish_fp8(workspace, slices, qkv, cos, sin, pos, kc, vc, ks, vs, B, H, hd, Smax):
    """qkv_finish with k / v quantised into the fp8 cache at `pos`: codes kc / vc uint8, scales ks / vs fp32  (egomi_qkv_finish_fp8)."""
    call("egomi_qkv_finish_fp8", workspace, slices, qkv, _ld(qkv), cos, sin, pos, kc, vc, ks, vs, B, H, hd, Smax, dt(qkv.dtype), S())


# ------------------------------------------------------------------------------------------ fp8 weights (decode projections)
def quantize_rows_fp8(w):
    """bf16 rows w [N, K] -> (codes uint8 [N, K], scales fp32 [N]): s_n = amax_n / 448 (1 where amax == 0), codes = e4m3fn(w / s_n)
    (egomi_quantize_rows_fp8; bit-equal to decode.kv8_quantize applied row-wise)."""
    if w.dtype != torch.bfloat16:
        raise TypeError("quantize_rows_fp8 takes bf16 rows")
    N, K = w.shape
    codes = torch.empty(N, K, dtype=torch.uint8, device=w.device)
    scales = torch.empty(N, dtype=torch.float32, device=w.device)
    call("egomi_quantize_rows_fp8", w, _ld(w), N, K, codes, K, scales, S())
    return codes, scales


def _wq_launch(sym, x, codes, scales, out, residual, workspace, epilogue):
    """egomi_gemm_w8 / egomi_gemm_w4 (one argument list: csrc/wq_gemm.h) on operands the format's caller has checked."""
    M, K = x.shape
    N = codes.shape[0]
    call(sym, x, _ld(x), codes, _ld(codes), scales, out, _ld(out) if out is not None else 0, residual, _ld(residual) if residual is not None else 0,
         M, N, K, epilogue, workspace, workspace.numel() * workspace.element_size() if workspace is not None else 0, S())


def _wq_slabs(launch, count_sym, x, codes, scales, workspace, count_only):
    """The slab path of either format: the library's count for this shape and workspace, then (unless count_only) the launch."""
    M, K = x.shape
    N = codes.shape[0]
    n = query(count_sym, M, N, K, workspace.numel() * workspace.element_size())
    if not count_only:
        launch(x, codes, scales, None, None, workspace, _abi.EGOMI_EPI_SLABS)
    return n


def _w8(x, codes, scales, out, residual, workspace, epilogue):
    K, N = x.shape[1], codes.shape[0]
    if x.dtype != torch.bfloat16 or codes.dtype != torch.uint8 or scales.dtype != torch.float32 or codes.shape[1] != K or scales.shape != (N,):
        raise TypeError("mm_w8: x bf16 [M, K], codes uint8 [N, K], scales fp32 [N]")
    _wq_launch("egomi_gemm_w8", x, codes, scales, out, residual, workspace, epilogue)


def mm_w8(x, codes, scales, out=None, residual=None, workspace=None):
    """out = bf16(x . (codes * scales[:, None])^T (+ residual)): x bf16 [M, K] with M <= 512, fp8 weights from quantize_rows_fp8
    (egomi_gemm_w8, EGOMI_EPI_NONE; `workspace` lets the library split K)."""
    if out is None:
        out = torch.empty(x.shape[0], codes.shape[0], dtype=torch.bfloat16, device=x.device)
    _w8(x, codes, scales, out, residual, workspace, _abi.EGOMI_EPI_NONE)
    return out


def mm_w8_slabs(x, codes, scales, workspace, count_only=False):
    """x . (codes * scales[:, None])^T as UNSUMMED fp32 K-slice slabs [slices, M, N] at the start of `workspace` (egomi_gemm_w8,
    EGOMI_EPI_SLABS); returns the number of slices (count_only: without launching; 0 = the library cannot run this shape)."""
    return _wq_slabs(_w8, "egomi_gemm_w8_slab_count", x, codes, scales, workspace, count_only)


# ------------------------------------------------------------------------------------------ int4 weights (decode projections)
def quantize_rows_int4(w):
    """bf16 rows w [N, K], K % 32 == 0 -> (packed uint8 [N, K / 2], scales fp32 [ceil(K / 128), N]): per row and 128-column group
    s = amax / 7 (1 where amax == 0), code = clamp(round(w / s), -7, 7), two codes per byte (column 2 b low, 2 b + 1 high)
    (egomi_quantize_rows_int4; bit-equal to decode.w4_quantize run on the host)."""
    if w.dtype != torch.bfloat16:
        raise TypeError("quantize_rows_int4 takes bf16 rows")
    N, K = w.shape
    packed = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
    scales = torch.empty(-(-K // 128), N, dtype=torch.float32, device=w.device)
    call("egomi_quantize_rows_int4", w, _ld(w), N, K, packed, K // 2, scales, S())
    return packed, scales


def _w4(x, packed, scales, out, residual, workspace, epilogue):
    K, N = x.shape[1], packed.shape[0]
    if x.dtype != torch.bfloat16 or packed.dtype != torch.uint8 or scales.dtype != torch.float32 or packed.shape[1] * 2 != K \
            or scales.shape != (-(-K // 128), N) or not scales.is_contiguous():
        raise TypeError("mm_w4: x bf16 [M, K], packed uint8 [N, K / 2], scales fp32 [ceil(K / 128), N] contiguous")
    _wq_launch("egomi_gemm_w4", x, packed, scales, out, residual, workspace, epilogue)


def mm_w4(x, packed, scales, out=None, residual=None, workspace=None):
    """out = bf16(x . dequantized(packed, scales)^T (+ residual)): x bf16 [M, K] with M <= 512, int4 weights from quantize_rows_int4
    (egomi_gemm_w4, EGOMI_EPI_NONE; `workspace` lets the library split K)."""
    if out is None:
        out = torch.empty(x.shape[0], packed.shape[0], dtype=torch.bfloat16, device=x.device)
    _w4(x, packed, scales, out, residual, workspace, _abi.EGOMI_EPI_NONE)
    return out


def mm_w4_slabs(x, packed, scales, workspace, count_only=False):
    """mm_w4's product as UNSUMMED fp32 K-slice slabs [slices, M, N] at the start of `workspace` (egomi_gemm_w4, EGOMI_EPI_SLABS);
    returns the number of slices (count_only: without launching; 0 = the library cannot run this shape)."""
    return _wq_slabs(_w4, "egomi_gemm_w4_slab_count", x, packed, scales, workspace, count_only)


# ------------------------------------------------------------------------------------------ rows
def layernorm(x, w, b, eps=1e-5, add=None, sum_out=None, out=None):
    rows, cols = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    call("egomi_layernorm_fwd", x, add, w, b, sum_out, out, rows, cols, eps, dt(x.dtype), S())
    return out


def rmsnorm(x, w, eps, rstd=None, out=None, tail=None, tail_residual=None):
    """tail = (row0, slices, slab address) from mm(..., defer_tail=True): rows >= row0 of x are formed here from the product's
    K-slice slabs (+ tail_residual's rows), written to x and normalised in one pass (egomi_rmsnorm_fwd_tail)."""
    rows, cols = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    if tail is not None:
        call("egomi_rmsnorm_fwd_tail", x, w, out, rstd, rows, cols, eps, tail[0], c_p(tail[2]), tail[1], tail_residual,
             _ld(tail_residual) if tail_residual is not None else 0, dt(x.dtype), S())
        return out
    call("egomi_rmsnorm_fwd", x, w, out, rstd, rows, cols, eps, dt(x.dtype), S())
    return out


def rmsnorm_bwd(dy, x, w, rstd, dx_add=None, dw=None, out=None, tail=None, window=None):
    """tail: as in rmsnorm() — dy's rows >= row0 are still the slabs of the dgrad product that made dy (egomi_rmsnorm_bwd_tail).
    window = (S, R): the operands hold the last R rows of every S-row sequence only; dw gets the bits of the full-layout call whose other
    rows have dy = 0 (egomi_rmsnorm_bwd_rows)."""
    rows, cols = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    if window is not None:
        call("egomi_rmsnorm_bwd_rows", dy, x, w, rstd, out, dx_add, dw, rows, cols, window[0], window[1], dt(x.dtype), S())
        return out
    if tail is not None:
        call("egomi_rmsnorm_bwd_tail", dy, x, w, rstd, out, dx_add, dw, rows, cols, tail[0], c_p(tail[2]), tail[1], dt(x.dtype), S())
        return out
    call("egomi_rmsnorm_bwd", dy, x, w, rstd, out, dx_add, dw, rows, cols, dt(x.dtype), S())
    return out


def rope_tables(seq, head_dim, theta):
    """fp32 cos/sin [S, hd/2], computed exactly as HF LlamaRotaryEmbedding does (modeling_llama.py:93-127)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    freqs = torch.arange(seq, dtype=torch.float32)[:, None] * inv[None, :]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def rope_(x, cos, sin, rows, seq, pos_offset, H, hd, ld, inverse=False):
    call("egomi_rope", x, cos, sin, rows, seq, pos_offset, H, hd, ld, int(inverse), dt(x.dtype), S())
    return x


def rope_qkv_tail_(qkv, cos, sin, rows, seq, pos_offset, H, hd, ld, tail):
    """rope_ on the q and k heads of a stacked q|k|v array (H = heads of ONE of them) whose rows >= tail[0] are still the K-slice
    slabs of the product (mm(..., defer_tail=True)): summed, rounded, rotated / materialised in this pass (egomi_rope_qkv_tail)."""
    call("egomi_rope_qkv_tail", qkv, cos, sin, rows, seq, pos_offset, H, hd, ld, tail[0], c_p(tail[2]), tail[1], dt(qkv.dtype), S())
    return qkv


def swiglu(gate, up, out):
    rows, cols = gate.shape
    call("egomi_swiglu_fwd", gate, up, out, rows, cols, _ld(gate), _ld(out), dt(gate.dtype), S())
    return out


def swiglu_il(gu, out):
    """Interleaved-32 gate|up array gu [rows, 2*cols] -> out [rows, cols] = silu(gate)*up."""
    rows, cols = out.shape
    call("egomi_swiglu_il_fwd", gu, out, rows, cols, _ld(gu), _ld(out), dt(gu.dtype), S())
    return out


def swiglu_il_bwd(dact, gu, dgu):
    rows, cols = dact.shape
    call("egomi_swiglu_il_bwd", dact, gu, dgu, rows, cols, _ld(gu), _ld(dact), _ld(dgu), dt(gu.dtype), S())
    return dgu


def gemm_kernel_id(M, N, K, dtype=torch.bfloat16, out_dtype=torch.bfloat16):
    """Which kernel egomi_gemm would pick for a plain contiguous NT product of this shape (2 = 256x256 8-phase)."""
    d = GemmDesc()
    d.A = d.B = d.C = 256                                 # aligned placeholders: the selection looks at shapes and alignment only
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, K, K, N
    d.ab_dtype, d.c_dtype, d.batch = dt(dtype), dt(out_dtype), 1
    return query("egomi_gemm_kernel_id", ctypes.byref(d))


def mm_kernel_id(a, b, out, a_layout=0, b_layout=0, accumulate=False):
    """Which kernel egomi_gemm would run for mm(a, b, out=out, a_layout=..., b_layout=...): 0 generic, 1 / 2 the K-contiguous tuned kernels,
    3 the k-major 8-phase kernel of csrc/gemm_tn.hip (weight gradients, data gradients against an un-transposed weight)."""
    M, K = (a.shape if a_layout == 0 else (a.shape[1], a.shape[0]))
    N = b.shape[0] if b_layout == 0 else b.shape[1]
    d = GemmDesc()
    d.A, d.B, d.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, _ld(a), _ld(b), _ld(out)
    d.a_layout, d.b_layout, d.ab_dtype, d.c_dtype, d.batch = a_layout, b_layout, dt(a.dtype), dt(out.dtype), 1
    d.alpha, d.accumulate = 1.0, int(accumulate)
    return query("egomi_gemm_kernel_id", ctypes.byref(d))


GEMM_FORMS = {0: "none", 1: "generic", 2: "128x128", 3: "256x128", 4: "gemv_m16", 5: "m256", 6: "8phase", 7: "persistent", 8: "tall",
              9: "split", 10: "kmajor", 11: "kmajor_tall", 12: "kmajor_split"}


def gemm_last_route():
    """The route of this thread's most recent egomi_gemm (include/egomi.h egomi_gemm_last_route), as recorded by the launch that ran:
    (form name, split-K slices, first K-sliced tail row, tail slices, column split Na)."""
    out = (c_i * 4)()
    form = query("egomi_gemm_last_route", out)
    if form < 0:
        _lib.check(form, "egomi_gemm_last_route")
    return (GEMM_FORMS[form],) + tuple(out)


def swiglu_bwd(dact, gate, up, dgate, dup):
    rows, cols = gate.shape
    call("egomi_swiglu_bwd", dact, gate, up, dgate, dup, rows, cols, _ld(gate), _ld(dact), _ld(dgate), dt(gate.dtype), S())


def gelu(x, out=None):
    out = torch.empty_like(x) if out is None else out
    call("egomi_gelu_fwd", x, out, x.numel(), dt(x.dtype), S())
    return out


def gelu_bwd(dy, x, out=None):
    out = torch.empty_like(x) if out is None else out
    call("egomi_gelu_bwd", dy, x, out, x.numel(), dt(x.dtype), S())
    return out


def softmax(scores, Z, heads, Sq, Sk, out, causal=False, q_offset=0, key_mask=None):
    call("egomi_softmax_fwd", scores, Sk, key_mask, Z, heads, Sq, Sk, int(causal), q_offset, out, Sk, dt(out.dtype), S())
    return out


def softmax_bwd(Pm, dP, dS, rows, Sk):
    call("egomi_softmax_bwd", Pm, Sk, dP, Sk, dS, Sk, rows, Sk, dt(Pm.dtype), S())
    return dS


def splice_scan(ids, tok, Pn, n_clouds=None):
    """-> (start_pos, err, cloud_idx), int32 [B] each (include/egomi.h: the reference's position checks and its running cloud index)."""
    B, Sl = ids.shape
    sp, err, cloud, scratch = (torch.empty(B, dtype=torch.int32, device=ids.device) for _ in range(4))
    call("egomi_splice_scan", ids, B, Sl, tok.point_patch, tok.point_start, tok.point_end, Pn, B if n_clouds is None else n_clouds, sp, err, cloud,
         scratch, S())
    return sp, err, cloud


def embed_splice(ids, W, feats, start_pos, Pn, out=None, cloud_idx=None):
    B, Sl = ids.shape
    V, d = W.shape
    out = torch.empty(B, Sl, d, dtype=W.dtype, device=W.device) if out is None else out
    call("egomi_embed_splice_fwd", ids, W, feats, start_pos, cloud_idx, B, Sl, d, Pn, V, out, dt(W.dtype), S())
    return out


def embed_splice_bwd(dout, ids, start_pos, Pn, V, dW=None, dfeats=None, cloud_idx=None):
    B, Sl, d = dout.shape
    call("egomi_embed_splice_bwd", dout, ids, start_pos, cloud_idx, B, Sl, d, Pn, V, dW, dfeats, dt(dout.dtype), S())


def cross_entropy(logits, targets, ignore_index, dlogits=None, grad_scale=1.0):
    """Returns (loss_sum fp32 [1], count i32 [1]); mean loss = loss_sum / count."""
    R, V = logits.shape
    cnt = torch.zeros(1, dtype=torch.int32, device=logits.device)
    ls = torch.zeros(1, dtype=torch.float32, device=logits.device)
    rows = torch.empty(R, dtype=torch.float32, device=logits.device)
    call("egomi_ce_count", targets, R, ignore_index, cnt, S())
    call("egomi_ce_fwd_bwd", logits, _ld(logits), targets, R, V, ignore_index, cnt, ls, rows, dlogits, _ld(dlogits) if dlogits is not None else 0,
         grad_scale, dt(logits.dtype), S())
    return ls, cnt


def cross_entropy_soft(logits, targets, ignore_index, spec, dlogits=None, grad_scale=1.0):
    """The same loss against the bin-aware target `spec` = (p0, nb, sigma, radius) (traj.soft_target_spec; include/egomi.h,
    egomi_ce_soft_fwd_bwd).  Returns (loss_sum fp32 [1], nll_sum fp32 [1], count i32 [1]): mean soft loss = loss_sum / count, mean hard
    loss (what cross_entropy returns for the same rows) = nll_sum / count."""
    R, V = logits.shape
    p0, nb, sigma, radius = spec
    cnt = torch.zeros(1, dtype=torch.int32, device=logits.device)
    sums = torch.zeros(2, dtype=torch.float32, device=logits.device)
    rows = torch.empty(2, R, dtype=torch.float32, device=logits.device)
    call("egomi_ce_count", targets, R, ignore_index, cnt, S())
    call("egomi_ce_soft_fwd_bwd", logits, _ld(logits), targets, R, V, ignore_index, cnt, p0, nb, sigma, radius, sums[0:1], sums[1:2], rows[0], rows[1],
         dlogits, _ld(dlogits) if dlogits is not None else 0, grad_scale, dt(logits.dtype), S())
    return sums[0:1], sums[1:2], cnt


def adamw(master, model_copy, grad, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, grad_scale_dev=None):
    """grad_scale_dev (a device fp32 scalar, clip_scale's out[2:3]): the scale is read on the device and `grad_scale` is not used."""
    if grad.dtype not in (torch.float32, torch.bfloat16) or not grad.is_contiguous() or grad.numel() != master.numel():
        raise _lib.EgomiError("adamw: the gradient must be a contiguous fp32 or bf16 tensor of the parameter's size")
    if grad_scale_dev is not None:
        if grad_scale_dev.dtype != torch.float32 or grad_scale_dev.numel() != 1:
            raise _lib.EgomiError("adamw: grad_scale_dev must be one fp32 value on the device")
        call("egomi_adamw_ds" if grad.dtype == torch.float32 else "egomi_adamw_g16_ds", master, model_copy, grad, m, v, master.numel(), lr, beta1,
             beta2, eps, wd, step, grad_scale_dev, dt(model_copy.dtype) if model_copy is not None else F32, S())
        return
    call("egomi_adamw" if grad.dtype == torch.float32 else "egomi_adamw_g16", master, model_copy, grad, m, v, master.numel(), lr, beta1, beta2, eps,
         wd, step, grad_scale, dt(model_copy.dtype) if model_copy is not None else F32, S())


def grad_sumsq_chunk():
    """Elements per stage-1 workgroup of grad_sumsq (a constant of the library)."""
    return query("egomi_grad_sumsq_chunk")


class GradTable:
    """The device-resident segment table of grad_sumsq for a list of contiguous fp32 / bf16 tensors, with its outputs and workspace.
    `key` is the tuple of (address, numel, dtype) it was built from: the caller rebuilds the table when that changes.  Building it
    copies three small host arrays to the device; using it never syncs."""

    def __init__(self, tensors):
        if not tensors:
            raise _lib.EgomiError("grad_sumsq: no gradient tensors")
        for g in tensors:
            if not g.is_cuda or g.dtype not in (torch.float32, torch.bfloat16) or not g.is_contiguous() or g.numel() <= 0:
                raise _lib.EgomiError("grad_sumsq: every segment must be a non-empty contiguous fp32 or bf16 device tensor")
        self.key = self.key_of(tensors)
        self.tensors = list(tensors)                            # the table holds addresses: keep what they point at alive
        dev, ch = tensors[0].device, grad_sumsq_chunk()
        self.n_seg = len(tensors)
        self.n_chunks = sum(-(-g.numel() // ch) for g in tensors)
        self.addr = torch.tensor([k[0] for k in self.key], dtype=torch.int64).to(dev)
        self.numel = torch.tensor([k[1] for k in self.key], dtype=torch.int64).to(dev)
        codes = [dt(k[2]) for k in self.key]
        self.dtype0 = codes[0]                                  # one dtype throughout (every table outside data parallelism): no dtype table
        self.dtype = None if len(set(codes)) == 1 else torch.tensor(codes, dtype=torch.int32).to(dev)
        self.seg_sumsq = torch.zeros(self.n_seg, dtype=torch.float64, device=dev)
        self.total = torch.zeros(1, dtype=torch.float64, device=dev)
        self.ws_bytes = query("egomi_grad_sumsq_workspace_bytes", self.n_seg, self.n_chunks)
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=dev)

    @staticmethod
    def key_of(tensors):
        return tuple((g.data_ptr(), g.numel(), g.dtype) for g in tensors)


def grad_sumsq(table):
    """table.seg_sumsq f64 [n_seg] and table.total f64 [1] of the table's segments: two launches, float64, no atomics (include/egomi.h)."""
    call("egomi_grad_sumsq", table.addr, table.numel, table.dtype, table.dtype0, table.n_seg, table.n_chunks, table.seg_sumsq, table.total, table.ws,
         table.ws_bytes, S())
    return table.seg_sumsq, table.total


def clip_scale(total_sumsq, grad_scale, max_norm, out, stats):
    """out f32 [3] = (total_norm, coef, effective grad scale); stats f64 [5] accumulated in place (include/egomi.h)."""
    call("egomi_clip_scale", total_sumsq, grad_scale, max_norm, out, stats, S())
    return out


def transpose(x, ldo=None, out=None):
    R, C = x.shape
    ldo = R if ldo is None else ldo
    out = torch.empty(C, ldo, dtype=x.dtype, device=x.device) if out is None else out
    call("egomi_transpose", x, R, C, _ld(x), out, ldo, dt(x.dtype), S())
    return out


def cast(x, dtype, out=None):
    out = torch.empty(x.shape, dtype=dtype, device=x.device) if out is None else out
    call("egomi_cast", x, dt(x.dtype), out, dt(dtype), x.numel(), S())
    return out


def rank_sum(chunks, out):
    """chunks [W, c] (bf16 / fp32, contiguous) -> out [c] (bf16 / fp32): fp32-accumulated sum over the leading (rank) axis."""
    W, c = chunks.shape
    call("egomi_rank_sum", chunks, dt(chunks.dtype), W, c, out, dt(out.dtype), S())
    return out


def add(a, b, out=None):
    out = torch.empty_like(a) if out is None else out
    call("egomi_add", a, b, out, a.numel(), dt(a.dtype), S())
    return out


def colsum_(x, out):
    """out (fp32 [C]) += column sums of x [R,C]."""
    R, C = x.shape
    call("egomi_colsum", x, R, C, _ld(x), out, dt(x.dtype), S())
    return out


def group_max(x, BG, M, C, concat=False, out=None):
    if out is None:
        out = torch.empty((BG * M, 2 * C) if concat else (BG, C), dtype=x.dtype, device=x.device)
    call("egomi_group_max", x, BG, M, C, out, int(concat), dt(x.dtype), S())
    return out


def linear_smallk(x, w, b, act=0, out=None):
    R, K = x.numel() // x.shape[-1], x.shape[-1]
    N = w.shape[0]
    out = torch.empty(R, N, dtype=w.dtype, device=w.device) if out is None else out
    call("egomi_linear_smallk", x, dt(x.dtype), w, b, out, R, N, K, act, dt(w.dtype), S())
    return out


# ------------------------------------------------------------------------------------------ fused attention
AttnDesc = _abi.STRUCTS["egomi_attn_desc"]


def _attn_desc(qkv, B, Sq, H, hd, scale, causal, key_mask):
    d = AttnDesc()
    dm = H * hd
    d.q, d.k, d.v = qkv[:, :dm].data_ptr(), qkv[:, dm:2 * dm].data_ptr(), qkv[:, 2 * dm:].data_ptr()
    d.key_mask = key_mask.data_ptr() if key_mask is not None else None
    d.B, d.H, d.S, d.head_dim = B, H, Sq, hd
    d.ld_qkv = qkv.stride(0)
    d.scale, d.causal, d.dtype = scale, int(causal), dt(qkv.dtype)
    return d


def attn_fwd(qkv, B, Sq, H, hd, scale, out, lse, causal=True, key_mask=None, q_rows=0):
    """qkv [B*S, 3*H*hd] (q|k|v column blocks) -> out [B*S, H*hd], lse fp32 [B,H,S].
    q_rows = R in (0, S): only rows >= S - R of out / lse are promised (include/egomi.h, egomi_attn_desc.q_rows)."""
    d = _attn_desc(qkv, B, Sq, H, hd, scale, causal, key_mask)
    d.q_rows = int(q_rows)
    d.o, d.lse, d.ld_o = out.data_ptr(), lse.data_ptr() if lse is not None else None, out.stride(0)
    call("egomi_attn_fwd", ctypes.byref(d), S())
    return out


def attn_bwd(qkv, out, lse, dout, dqkv, delta, B, Sq, H, hd, scale, causal=True, key_mask=None, rope=None, q_rows=0):
    """dq|dk|dv written into the column blocks of dqkv [B*S, 3*H*hd]; delta fp32 [B,H,S] is scratch.
    rope=(cos, sin) fp32 [>=S, hd/2]: dq and dk come out rotated back (== rope_(dqkv, inverse=True) afterwards).
    q_rows = R in (0, S): the caller promises dout == 0 at rows < S - R; dq|dk|dv are what q_rows = 0 gives, at every row."""
    d = _attn_desc(qkv, B, Sq, H, hd, scale, causal, key_mask)
    d.q_rows = int(q_rows)
    if rope is not None:
        cos, sin = rope
        if cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.shape[0] < Sq or cos.shape[1] != hd // 2 \
                or not cos.is_contiguous() or not sin.is_contiguous():
            raise ValueError("attn_bwd: rope tables must be contiguous fp32 [>=S, head_dim/2]")
        d.rope_cos, d.rope_sin = cos.data_ptr(), sin.data_ptr()
    dm = H * hd
    d.o, d.lse, d.ld_o = out.data_ptr(), lse.data_ptr(), out.stride(0)
    if dout.stride(0) != out.stride(0):
        raise ValueError("attn_bwd: dout and out must share their row stride")
    d.dout, d.delta = dout.data_ptr(), delta.data_ptr()
    d.dq, d.dk, d.dv = dqkv[:, :dm].data_ptr(), dqkv[:, dm:2 * dm].data_ptr(), dqkv[:, 2 * dm:].data_ptr()
    d.ld_dqkv = dqkv.stride(0)
    call("egomi_attn_bwd", ctypes.byref(d), S())
    return dqkv


# ------------------------------------------------------------------------------------------ LoRA (csrc/lora.hip)
# PEFT's lora.Linear.forward: y = x W^T + s (x A^T) B^T, s = lora_alpha / r (no dropout, no bias).  `il`: the wide activation operand is
# read / written in the interleaved-32 gate|up layout (include/egomi.h).
def lora_down_workspace_bytes(M, K, R):
    return query("egomi_lora_down_workspace_bytes", M, K, R)


def lora_down(x, q, out, q_trans=False, il=False, alpha=1.0, workspace=None):
    """out [M, R] = alpha * x [M, K] . Q^T with Q [R, K] (q_trans: Q given as q = Q^T [K, R]).  T = x A^T (A stacked over the adapters
    that share x), or U = dY B (q = B, q_trans=True).  workspace: a uint8 tensor of at least lora_down_workspace_bytes(M, K, R) bytes
    (allocated here when too small)."""
    R, K = (q.shape[1], q.shape[0]) if q_trans else (q.shape[0], q.shape[1])
    M = out.shape[0]
    if out.shape[1] != R or x.dtype != q.dtype or out.dtype != q.dtype or q.stride(1) != 1 or x.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError("lora_down: x [M, K], Q [R, K] (or Q^T), out [M, R] of one dtype, rows contiguous")
    if x.shape[0] < M or x.shape[1] < (2 * K - 32 if il else K):
        raise ValueError(f"lora_down: x {tuple(x.shape)} is smaller than [{M}, {2 * K - 32 if il else K}] (M rows, K logical columns)")
    need = lora_down_workspace_bytes(M, K, R) if R % 8 == 0 and 8 <= R <= 192 else 0
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        workspace = torch.empty(need, dtype=torch.uint8, device=out.device)
    wb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    call("egomi_lora_down", x, x.stride(0), q, q.stride(0), int(q_trans), out, out.stride(0), M, K, R, alpha, int(il), workspace, wb, dt(x.dtype),
         S())
    return out


def lora_up(p, q, out, alpha, q_trans=False, il=False):
    """out [M, N] += alpha * p [M, R] . Q^T with Q [N, R] (q_trans: Q given as q = Q^T [R, N]); one fp32 sum, rounded once.
    y += s T B^T (q = B), dX += s U A (q = A, q_trans=True), merging W += s B A (p = B, q = A, q_trans=True)."""
    M, R = p.shape
    N = q.shape[1] if q_trans else q.shape[0]
    if (q.shape[0] if q_trans else q.shape[1]) != R or p.dtype != q.dtype or out.dtype != q.dtype or \
            p.stride(1) != 1 or q.stride(1) != 1 or out.stride(1) != 1 or out.shape[0] != M:
        raise ValueError("lora_up: p [M, R], Q [N, R] (or Q^T), out [M, >= N] of one dtype, rows contiguous")
    if out.shape[1] < (2 * N - 32 if il else N):
        raise ValueError(f"lora_up: out {tuple(out.shape)} is narrower than {2 * N - 32 if il else N} columns")
    call("egomi_lora_up", p, p.stride(0), q, q.stride(0), int(q_trans), out, out.stride(0), M, N, R, alpha, int(il), dt(p.dtype), S())
    return out


def lora_wgrad_workspace_bytes(M, Pd, Qd):
    return query("egomi_lora_wgrad_workspace_bytes", M, Pd, Qd)


def lora_wgrad(l, r, g, alpha, accumulate=False, il=False, Pd=None, workspace=None):
    """g fp32 [P, Q] (+)= alpha * l[:, :P]^T . r [M, Q], summed over M in a fixed order: dA = s U^T x (l = U), dB = s dY^T T (l = dY).
    Pd: the logical width of l (default g's rows).  workspace: a uint8 tensor of at least lora_wgrad_workspace_bytes(M, P, Q) bytes."""
    M, Qd = r.shape
    Pd = g.shape[0] if Pd is None else Pd
    if g.dtype != torch.float32 or g.shape[1] != Qd or g.stride(1) != 1 or l.dtype != r.dtype or l.stride(1) != 1 or r.stride(1) != 1 \
            or l.shape[0] != M:
        raise ValueError("lora_wgrad: l [M, >= P], r [M, Q] of one dtype, g fp32 [P, Q], rows contiguous")
    if g.shape[0] != Pd or l.shape[1] < (2 * Pd - 32 if il else Pd):
        raise ValueError(f"lora_wgrad: l {tuple(l.shape)} is narrower than {2 * Pd - 32 if il else Pd} columns, or g has not {Pd} rows")
    need = lora_wgrad_workspace_bytes(M, Pd, Qd)
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        workspace = torch.empty(need, dtype=torch.uint8, device=g.device)
    wb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    call("egomi_lora_wgrad", l, l.stride(0), r, r.stride(0), g, g.stride(0), M, Pd, Qd, alpha, int(accumulate), int(il), workspace, wb, dt(r.dtype),
         S())
    return g
