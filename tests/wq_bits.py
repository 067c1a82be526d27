"""The bits of the quantized decode-weight products (csrc/w8.hip, csrc/w4.hip, csrc/wq_gemm.h: egomi_gemm_w8, egomi_gemm_w4), as data.

Inputs come from a fixed 32-bit integer hash in int64 tensor arithmetic on the host, so they depend on no random generator and no torch
version; the codes are fed to the products directly (the quantizers are not under test).  digests() runs one (format, N, K, M) case in
the three forms a decode step uses and returns the SHA-256 of each result's raw bytes.  tests/golden/wq_gemm_bits.json holds them as
recorded by tools/debug/record_wq_bits.py on the commit named in the file, before the two formats shared any code;
tests/test_gpu_wq_bits.py asserts them, so a reordered fp32 sum anywhere in the products shows.  grid_counts() is the host-only part:
the slab counts of tests/golden/wq_slab_counts.json (tests/test_wq_plan_host.py)."""
import hashlib

import torch

# (N, K): tests/test_gpu_w4_kernels.SMALL (single ragged group, clamped rows, full tile and group, 32-wide last group, split 2 and 4), and
# (132, 2144): K / 32 = 67 units, so at most 4 slices = 16 slots of one 128-deep step each, a 96-wide tail on the last slot, N % 64 != 0
SHAPES = [(4, 32), (60, 96), (64, 128), (68, 160), (704, 352), (384, 1024), (132, 2144)]
MS = [1, 3, 16, 17, 40]                                                   # MT = 1 and 2, ragged M-chunks
FORMATS = ("w8", "w4")
WS_BYTES = 64 << 20
MASK = 0xFFFFFFFF


def h(rows, cols, seed):
    """uint32 hash of (row, col, seed) as an int64 tensor [rows, cols]; every intermediate stays below 2^63."""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    v = (r * 0x9E3779B1 + c * 0x85EBCA77 + seed * 0xC2B2AE3D) & MASK
    v = v ^ (v >> 15)
    v = (v * 0x2C1B3C6D) & MASK
    v = v ^ (v >> 12)
    v = (v * 0x297A2D39) & MASK
    return v ^ (v >> 15)


def inputs(fmt, N, K, M):
    """x bf16 [M, K], residual bf16 [M, N], codes uint8, scales fp32 in `fmt`'s layout (csrc/w8.hip, csrc/w4.hip), on the host."""
    x = ((h(M, K, 1) % 513 - 256).float() / 64).to(torch.bfloat16)
    res = ((h(M, N, 2) % 513 - 256).float() / 8).to(torch.bfloat16)
    if fmt == "w8":
        codes = h(N, K, 3) % 256
        codes = torch.where((codes & 0x7F) == 0x7F, codes - 1, codes).to(torch.uint8)       # the two NaN bytes -> 0x7E / 0xFE
        scales = (2.0 ** -10 * (1 + (h(N, 1, 4) % 1024).float() / 1024))[:, 0].contiguous()
    else:
        nib = 1 + h(N, K, 5) % 15
        codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8).contiguous()
        scales = (2.0 ** -10 * (1 + (h(-(-K // 128), N, 6) % 1024).float() / 1024)).contiguous()
    return x, res, codes, scales


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def key(fmt, N, K, M):
    return f"{fmt}/N{N}/K{K}/M{M}"


def digests(fmt, N, K, M, ws):
    """{"none": EPI_NONE without workspace, "res_ws": EPI_NONE with residual and workspace (planned split + reduce kernel),
    "slabs_n" / "slabs": EPI_SLABS' count and its fp32 slabs [n, M, N]}."""
    from egoscaler_amd import ops
    mm, mm_slabs = (ops.mm_w8, ops.mm_w8_slabs) if fmt == "w8" else (ops.mm_w4, ops.mm_w4_slabs)
    x, res, codes, scales = (t.cuda() for t in inputs(fmt, N, K, M))
    out = {"none": sha(mm(x, codes, scales)), "res_ws": sha(mm(x, codes, scales, residual=res, workspace=ws))}
    ws.zero_()
    n = mm_slabs(x, codes, scales, ws)
    out["slabs_n"] = n
    out["slabs"] = sha(ws[:n * M * N * 4])
    return out


# ---------------------------------------------------------------------------------------------------- the plan, host only
PLAN_MS = [1, 8, 16, 17, 64, 512, 513]
# q|k|v, o_proj, gate|up, down_proj of config.dims_tiny (128 / 352) and dims_7b (4096 / 11008); N = 4 with one unit; N % 4; K % 32
PLAN_SHAPES = [(384, 128), (128, 128), (704, 128), (128, 352), (12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008),
               (4, 32), (66, 128), (128, 100)]


def plan_workspaces(M, N):
    slab = M * N * 4
    return [0, slab - 1, slab, 3 * slab + 1, 64 << 20]


def grid_counts(lib, fmt):
    """{"M/N/K/workspace bytes": egomi_gemm_<fmt>_slab_count} over the grid above."""
    import ctypes
    f = getattr(lib, f"egomi_gemm_{fmt}_slab_count")
    f.restype = ctypes.c_int
    return {f"{M}/{N}/{K}/{wb}": f(ctypes.c_int(M), ctypes.c_int(N), ctypes.c_int(K), ctypes.c_int64(wb))
            for M in PLAN_MS for N, K in PLAN_SHAPES for wb in plan_workspaces(M, N)}
