"""GPU: cached decoding (A13 / BASELINE config 5 mechanics): kv_append + attn_decode + argmax against
torch references, hipGraph-captured multi-step greedy decode == eager step-by-step decode == the
reference golden sequences."""
import os
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import synth
from egoscaler_amd.config import dims_tiny

pytestmark = pytest.mark.gpu


def _model(dims, dtype):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=dtype)
    sd = synth.synth_state_dict(dims, 0)
    m.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()})
    return m.eval()


@pytest.mark.parametrize("dtype,hd", [(torch.float32, 32), (torch.bfloat16, 128), (torch.bfloat16, 64)])
def test_kv_append_attn_decode_argmax(dtype, hd):
    from egoscaler_amd import decode as D
    B, H, Smax, T = 3, 2, 50, 37
    d = H * hd
    g = torch.Generator().manual_seed(hd)
    qkv = torch.randn(B, 3 * d, generator=g).to(dtype)
    K = torch.randn(B, T, d, generator=g).to(dtype)
    V = torch.randn(B, T, d, generator=g).to(dtype)
    kc = torch.zeros(B, H, Smax, hd, dtype=dtype, device="cuda")
    vc = torch.zeros_like(kc)
    kvrows = torch.cat([torch.zeros(B * T, d, dtype=dtype), K.reshape(B * T, d), V.reshape(B * T, d)], 1).cuda()
    D.kv_append(kvrows[:, d:2 * d], kvrows[:, 2 * d:], 3 * d, kc, vc, B, T - 1, H, hd, Smax, 0)         # rows of sample b are b*(T-1)+s
    # append semantics: write T-1 rows at 0, then the last row at position T-1 from a [B,1] step buffer
    Kc = K[:, :T - 1].reshape(B * (T - 1), d)
    Vc = V[:, :T - 1].reshape(B * (T - 1), d)
    rows = torch.cat([torch.zeros(B * (T - 1), d, dtype=dtype), Kc, Vc], 1).cuda()
    D.kv_append(rows[:, d:2 * d], rows[:, 2 * d:], 3 * d, kc, vc, B, T - 1, H, hd, Smax, 0)
    step = torch.cat([qkv[:, :d], K[:, T - 1], V[:, T - 1]], 1).cuda()
    D.kv_append(step[:, d:2 * d], step[:, 2 * d:], 3 * d, kc, vc, B, 1, H, hd, Smax, T - 1)
    assert torch.equal(kc[:, :, :T].cpu(), K.view(B, T, H, hd).transpose(1, 2)) and torch.equal(vc[:, :, :T].cpu(), V.view(B, T, H, hd).transpose(1, 2))
    km = torch.ones(B, Smax, dtype=torch.uint8)
    km[1, 5:9] = 0
    out = torch.zeros(B, d, dtype=dtype, device="cuda")
    D.attn_decode(step, 3 * d, kc, vc, km.cuda(), out, B, H, hd, Smax, T, hd ** -0.5)
    q = qkv[:, :d].float().view(B, H, 1, hd)
    kk, vv = K.float().view(B, T, H, hd).transpose(1, 2), V.float().view(B, T, H, hd).transpose(1, 2)
    sc = (q @ kk.transpose(-1, -2)) * hd ** -0.5
    sc = sc.masked_fill(~km[:, None, None, :T].bool(), float("-inf"))
    ref = (torch.softmax(sc, -1) @ vv).reshape(B, d)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert float((out.float().cpu() - ref).abs().max()) <= tol * float(ref.abs().max())
    lg = torch.randn(B, 1000, generator=g).to(dtype)
    lg[0, 17] = lg[0, 500] = 50.0                                     # tie: lowest index wins
    ids = torch.zeros(B, dtype=torch.int64, device="cuda")
    seq = torch.zeros(B, 9, dtype=torch.int64, device="cuda")
    D.argmax_rows(lg.cuda(), ids, seq, 4)
    want = lg.float().argmax(-1)
    want[0] = 17
    assert torch.equal(ids.cpu(), want) and torch.equal(seq[:, 4].cpu(), want) and int(seq.sum()) == int(want.sum())


def test_graph_captured_decode_equals_eager_and_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_model.npz"), allow_pickle=False)
    dims = dims_tiny()
    toks, masks, Lp = synth.synth_batch(dims, 2, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(2)])
    m = _model(dims, torch.float32)
    kw = dict(input_ids=toks[:, :Lp].cuda(), attention_mask=masks[:, :Lp].cuda(), point_clouds=pts.cuda(), max_length=10, do_sample=False,
              fps_start=g["fps_start"])
    og = m.generate(use_graph=True, **kw)
    oe = m.generate(use_graph=False, **kw)
    assert torch.equal(og.sequences, oe.sequences)
    assert np.array_equal(og.sequences.cpu().numpy(), g["gen_sequences"]), "hipGraph-captured greedy decode must reproduce the reference ids"
    sg, se = torch.stack(og.scores, 1).cpu(), torch.stack(oe.scores, 1).cpu()
    assert torch.equal(sg, se)
    assert float(np.abs(sg.numpy() - g["gen_scores"]).max()) < 1e-3 * float(np.abs(g["gen_scores"]).max())


def test_padded_prompts_decode_matches_full_forward():
    """Left-over padding inside the prompt batch: decode with the key mask must equal re-running the
    full forward on the grown sequence (bf16, head_dim 128 -> fused prefill + attn_decode)."""
    dims = dims_tiny()
    dims.lm.hidden_size, dims.lm.num_attention_heads, dims.lm.intermediate_size = 256, 2, 512
    toks, masks, Lp = synth.synth_batch(dims, 2, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(2)])
    m = _model(dims, torch.bfloat16)
    pm = masks[:, :Lp].clone()
    pm[1, 2:4] = False                                                # two masked prompt positions in sample 1
    o = m.generate(input_ids=toks[:, :Lp].cuda(), attention_mask=pm.cuda(), point_clouds=pts.cuda(), max_length=3, do_sample=False, fps_start=[0, 17])
    seq = o.sequences
    full_mask = torch.cat([pm, torch.ones(2, 2, dtype=torch.bool)], 1)
    with torch.no_grad():
        lg = m(input_ids=seq[:, :Lp + 2], attention_mask=full_mask.cuda(), point_clouds=pts.cuda(), fps_start=[0, 17]).logits[:, -1].float()
    ref = o.scores[2]
    assert float((lg - ref).abs().max()) <= 5e-2 * float(ref.abs().max())


@pytest.mark.parametrize("M,N,K", [(256, 8192, 4096), (256, 12288, 4096), (200, 8200, 2112), (129, 9000, 1024), (256, 32262, 4096), (256, 22016, 4096)])
def test_m256_ring_kernel_matches_reference(M, N, K):
    """gemm_nt_bf16_m256_kernel (128 < M <= 256: all rows x 128 columns per block, 3-stage LDS ring; the projections of the bs = 256 decode
    step) against the fp32 product of the same bf16 operands: plain, every epilogue form, fp32 output, explicit and planned K-splits, unsummed
    slabs (EGOMI_EPI_SLABS) — and bit-equality with the 128x128 kernel's result where the summation order is the same (no split)."""
    import ctypes
    from egoscaler_amd import ops, _lib
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    A, W = a.cuda(), w.cuda()
    ref = a.float() @ w.float().t()
    tol = 2e-2
    ws = torch.empty(128 << 20, dtype=torch.uint8, device="cuda")
    out = ops.mm(A, W)                                                        # no workspace: unsplit
    assert float((out.float().cpu() - ref).abs().max()) <= tol * float(ref.abs().max())
    out_ws = ops.mm(A, W, workspace=ws)                                       # the library's split plan + combine pass
    assert float((out_ws.float().cpu() - ref).abs().max()) <= tol * float(ref.abs().max())
    out32 = ops.mm(A, W, out_dtype=torch.float32, workspace=ws, split_k=3)
    assert float((out32.cpu() - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    if N % 8 == 0:
        bias = torch.randn(N, generator=g).bfloat16().cuda()
        res = torch.randn(M, N, generator=g).bfloat16().cuda()
        full = ops.mm(A, W, bias=bias, residual=res, act=ops.ACT_GELU, alpha=0.5, workspace=ws)
        want = torch.nn.functional.gelu(0.5 * ref + bias.float().cpu()) + res.float().cpu()
        assert float((full.float().cpu() - want).abs().max()) <= tol * float(want.abs().max())
    if N % 4 == 0:
        n = ops.mm_slabs(A, W, out, ws, count_only=True)
        if n >= 2:
            n2 = ops.mm_slabs(A, W, out, ws)
            assert n2 == n
            slabs = torch.frombuffer(ws.cpu().numpy().tobytes(), dtype=torch.float32)[:n * M * N].view(n, M, N)
            assert float((slabs.sum(0) - ref).abs().max()) <= 2e-3 * float(ref.abs().max())


@pytest.mark.parametrize("M,N,K,sk", [(256, 4096, 4096, 0), (256, 1024, 11008, 8), (64, 512, 512, 4), (300, 2018, 384, 3)])
def test_split_k_gemm_matches_unsplit(M, N, K, sk):
    """Skinny-M products with the K range split over blocks (fp32 slabs + combine) == the unsplit kernel."""
    from egoscaler_amd import ops
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, K, generator=g).bfloat16().cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16().cuda()
    bias = torch.randn(N, generator=g).bfloat16().cuda()
    res = torch.randn(M, N, generator=g).bfloat16().cuda()
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    ref = ops.mm(a, w, bias=bias, residual=res, act=ops.ACT_GELU, alpha=0.5)
    got = ops.mm(a, w, bias=bias, residual=res, act=ops.ACT_GELU, alpha=0.5, workspace=ws, split_k=sk)
    assert float((got.float() - ref.float()).abs().max()) <= 2e-2 * float(ref.float().abs().max())
    tiny_ws = torch.empty(1024, dtype=torch.uint8, device="cuda")          # too small for a slab: silently unsplit
    got2 = ops.mm(a, w, bias=bias, residual=res, act=ops.ACT_GELU, alpha=0.5, workspace=tiny_ws, split_k=sk)
    assert torch.equal(got2, ref)


def test_generate_reuses_its_decoder_and_captured_loop_across_calls():
    """run_validation / evaluate call generate() once per batch (train.py:223-228, evaluate.py:116-121).  Round 4: in frozen-LLM mode the Decoder
    (static KV cache, stacked weights) and the captured token loop are kept per geometry and REPLAYED by the next call.  A replay with other
    prompts, key masks and clouds gives exactly what a fresh decoder gives; results handed out earlier are copies (not views of the static
    buffers); a different geometry or sampling mode captures anew; EGOMI_DECODER_CACHE=0 restores one decoder per call."""
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16)
    toks, masks, Lp = synth.synth_batch(dims, 4, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(4)]).cuda()

    def gen(sel, T=5, **kw):
        pm = masks[sel, :Lp].clone()
        if kw.pop("pad_one", False):
            pm[0, 2:4] = False
        return m.generate(input_ids=toks[sel, :Lp].cuda(), attention_mask=pm.cuda(), point_clouds=pts[sel], max_length=T, do_sample=False,
                          fps_start=[0, 17][:len(sel)], eos_token_id=None, **kw)
    os.environ["EGOMI_DECODER_CACHE"] = "0"
    try:
        fresh_a, fresh_b = gen([0, 1]), gen([2, 3], pad_one=True)
        assert not m.__dict__.get("_decoders")
    finally:
        os.environ.pop("EGOMI_DECODER_CACHE")
    a = gen([0, 1])
    dec = next(iter(m._decoders.values()))
    assert len(m._decoders) == 1 and len(dec._graphs) == 1
    a_seq, a_sc = a.sequences.clone(), [s.clone() for s in a.scores]
    b = gen([2, 3], pad_one=True)                                          # same geometry: the same Decoder, the same graph, replayed
    assert next(iter(m._decoders.values())) is dec and len(dec._graphs) == 1
    assert torch.equal(a.sequences, a_seq) and all(torch.equal(x, y) for x, y in zip(a.scores, a_sc))     # earlier outputs were not overwritten
    assert torch.equal(a.sequences, fresh_a.sequences) and torch.equal(b.sequences, fresh_b.sequences)
    for x, y in zip(b.scores, fresh_b.scores):
        assert torch.equal(x, y)
    gen([0, 1], T=3)                                                       # another length: a second decoder
    assert len(m._decoders) == 2
    s1 = m.generate(input_ids=toks[:2, :Lp].cuda(), attention_mask=masks[:2, :Lp].cuda(), point_clouds=pts[:2], max_length=5, do_sample=True, fps_start=[0, 17], seed=3)
    s2 = m.generate(input_ids=toks[:2, :Lp].cuda(), attention_mask=masks[:2, :Lp].cuda(), point_clouds=pts[:2], max_length=5, do_sample=True, fps_start=[0, 17], seed=3)
    assert torch.equal(s1.sequences, s2.sequences)                         # the replayed sampling loop reads the seed from device memory
    assert len(dec._graphs) >= 2                                           # greedy and sampled loops are different captures of the same decoder


@pytest.mark.parametrize("M,N,K", [(8, 12288, 4096), (8, 4096, 4096), (16, 22016, 4096), (8, 4096, 11008), (1, 32262, 4096), (5, 200, 1024), (16, 4100, 1152)])
def test_gemv_m16_kernel_matches_reference(M, N, K):
    """gemv_m16_kernel (round 4: M <= 16, the decode projections at the reference's evaluation batch size — weight rows streamed from HBM to
    registers, x as the other MFMA operand, K cut over slices x 4 waves) against the fp32 product of the same bf16 operands: unsplit, the
    library's split plan + combine pass, an explicit split with fp32 output, the full epilogue, unsummed slabs (EGOMI_EPI_SLABS), ragged N,
    one row; EGOMI_GEMM_GEMV=0 is read once per process, so the A/B against the 128x128 kernel lives in tools/debug/validation_throughput.py."""
    from egoscaler_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    A, W = a.cuda(), w.cuda()
    ref = a.float() @ w.float().t()
    tol = 2e-2
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    out = ops.mm(A, W)                                                        # no workspace: every K slice in one block
    assert float((out.float().cpu() - ref).abs().max()) <= tol * float(ref.abs().max())
    out_ws = ops.mm(A, W, workspace=ws)                                       # the library's plan (split + combine where N is small)
    assert float((out_ws.float().cpu() - ref).abs().max()) <= tol * float(ref.abs().max())
    if N % 4 == 0:
        out32 = ops.mm(A, W, out_dtype=torch.float32, workspace=ws, split_k=3)
        assert float((out32.cpu() - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    bias = torch.randn(N, generator=g).bfloat16().cuda()
    res = torch.randn(M, N, generator=g).bfloat16().cuda()
    full = ops.mm(A, W, bias=bias, residual=res, act=ops.ACT_GELU, alpha=0.5, workspace=ws)
    want = torch.nn.functional.gelu(0.5 * ref + bias.float().cpu()) + res.float().cpu()
    assert float((full.float().cpu() - want).abs().max()) <= tol * float(want.abs().max())
    if N % 4 == 0:
        n = ops.mm_slabs(A, W, out, ws, count_only=True)
        if n >= 2:
            assert ops.mm_slabs(A, W, out, ws) == n
            slabs = torch.frombuffer(ws.cpu().numpy().tobytes(), dtype=torch.float32)[:n * M * N].view(n, M, N)
            assert float((slabs.sum(0) - ref).abs().max()) <= 2e-3 * float(ref.abs().max())


def test_attn_decode_bad_arguments_are_refused():
    """egomi_attn_decode / egomi_attn_decode_rows refuse a bad call on the host, before any launch, with the code include/egomi.h names:
    a NULL pointer or another dtype is a bad argument, a length or stride that does not fit is a shape error, another head_dim is
    unsupported (and is looked at only after the shapes)."""
    import ctypes
    from egoscaler_amd._lib import c_f, c_i, c_i64, lib
    from egoscaler_amd.ops import P, S
    E_BADARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -4
    L = lib()
    L.egomi_attn_decode.restype = L.egomi_attn_decode_rows.restype = ctypes.c_int
    B, H, hd, Smax = 2, 2, 64, 16
    d = H * hd
    x = torch.zeros(B, 3 * d, dtype=torch.bfloat16, device="cuda")
    kc = torch.zeros(B, H, Smax, hd, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(B, d, dtype=torch.bfloat16, device="cuda")
    mask = torch.ones(B, Smax, dtype=torch.uint8, device="cuda")
    tab = torch.zeros(B, Smax, dtype=torch.int32, device="cuda")
    nul = ctypes.c_void_p(None)

    def att(q=P(x), c=P(kc), v=P(kc), o=P(out), m=nul, ldm=0, T=4, dt=1, hd_=hd, ldq=3 * d, ldo=d, B_=B):
        return L.egomi_attn_decode(q, c_i64(ldq), c, v, m, c_i64(ldm), o, c_i64(ldo), c_i(B_), c_i(H), c_i(hd_), c_i(Smax), c_i(T), c_f(0.1), c_i(dt),
                                   S())

    def rws(q=P(x), c=P(kc), v=P(kc), o=P(out), tb=P(tab), ldkv=Smax, m=nul, ldm=0, T=4, nb=2, n_phys=B, dt=1, hd_=hd, ldq=3 * d, ldo=d, B_=B):
        return L.egomi_attn_decode_rows(q, c_i64(ldq), c, v, tb, c_i64(ldkv), c_i(n_phys), m, c_i64(ldm), o, c_i64(ldo), c_i(B_), c_i(nb), c_i(H),
                                        c_i(hd_), c_i(Smax), c_i(T), c_f(0.1), c_i(dt), S())

    for f in (att, rws):
        assert f(q=nul) == E_BADARG and f(c=nul) == E_BADARG and f(v=nul) == E_BADARG and f(o=nul) == E_BADARG
        assert f(B_=0) == E_SHAPE and f(ldo=d - 8) == E_SHAPE
        assert f(T=0) == E_SHAPE and f(T=Smax + 1) == E_SHAPE
        assert f(ldq=3 * d + 4) == E_SHAPE and f(ldq=d - 8) == E_SHAPE
        assert f(m=P(mask), ldm=3) == E_SHAPE
        assert f(hd_=48) == E_UNSUPPORTED and f(hd_=48, T=0) == E_SHAPE
        assert f(dt=5) == E_BADARG and f(dt=5, hd_=48) == E_BADARG
    assert rws(tb=nul) == E_BADARG
    assert rws(nb=3) == E_SHAPE and rws(n_phys=0) == E_SHAPE and rws(ldkv=3) == E_SHAPE
