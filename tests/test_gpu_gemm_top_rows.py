"""GPU: the route the windowed top decoder layer asks for (egomi_gemm with split_k = 1 at few tiles: whole 256x256 tiles on the 8-phase
kernel, csrc/gemm_fast.hip tile_choice) — the (M = 8 x 153 = 1224, N = 4096) products, which the rule moved off the 128x128 kernel and off
all-rows K-slicing.
  * against the float64 oracle of tests/gemm_oracle.py under its per-element bound, plain and with the residual epilogue (K cut to
    2048 / 4096 so that a case stays in seconds);
  * the property the engine relies on: a row of the M = 1224 product has the bits the same row has in the M = 5536 product of the library's
    default route (352x256 form, column split), for the six products of a layer with their epilogues at the bench step's shapes."""
import pytest
import torch

from tests.test_gpu_gemm_oracle import run_case

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, S, R = 8, 692, 153


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from egoscaler_amd import ops as O
    return O


@pytest.mark.parametrize("N,K,fam,epi", [(4096, 4096, "graded", ()), (4096, 2048, "exact", ("residual",)), (4096, 4096, "cancel", ("residual",)),
                                          (2048, 2048, "graded", ("residual",))])
def test_whole_tile_route_against_float64(ops, N, K, fam, epi):
    route, _, _, _ = run_case(ops, B * R, N, K, fam=fam, epi=epi, ws_kind="ws", split_k=1, form="8phase", tail=False, splitk=False)
    assert route[0] == "8phase" and route[3] == 0, route


def _rows(t):
    return t.view(B, S, -1)[:, S - R:].reshape(B * R, -1).contiguous()


@pytest.mark.parametrize("N,K,epi", [(4096, 4096, "residual"), (22016, 4096, "swiglu"), (4096, 11008, "residual"), (11008, 4096, "swiglu_bwd"),
                                     (4096, 22016, "none"), (4096, 4096, "none")])
def test_window_rows_keep_the_bits_of_the_full_product(ops, N, K, epi):
    g = torch.Generator(device="cuda").manual_seed(N + K)
    a = torch.randn(B * S, K, device="cuda", generator=g).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF)
    outs = []
    for M, pick, kw in ((B * S, lambda t: t, {}), (B * R, _rows, {"split_k": 1})):
        x = pick(a)
        c = torch.full((M, 2 * N if epi == "swiglu_bwd" else N), 7.0, dtype=BF, device="cuda")
        c2 = None
        if epi == "residual":
            kw["residual"] = pick(torch.randn(B * S, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)).to(BF))
        elif epi == "swiglu":
            c2 = kw["swiglu_out"] = torch.full((M, N // 2), 7.0, dtype=BF, device="cuda")
        elif epi == "swiglu_bwd":
            kw["swiglu_bwd_gu"] = pick(torch.randn(B * S, 2 * N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)).to(BF))
        ops.mm(x, w, out=c, **kw)
        torch.cuda.synchronize()
        outs.append((c, c2, ops.gemm_last_route()))
    (cf, c2f, rf), (cw, c2w, rw) = outs
    assert rw[0] == "8phase" and rw[3] == 0, rw                          # whole tiles: no K-sliced rows
    assert torch.equal(_rows(cf), cw), (rf, rw)
    if c2f is not None:
        assert torch.equal(_rows(c2f), c2w), (rf, rw)
    assert bool(torch.isfinite(cw.float()).all())
