"""MXFP4 weight-only skinny GEMM (csrc/kernels/mx4_gemm.hip) against fp32 on the CPU.

The oracle matrix is e2m1 grid values times per-block powers of two spread over 12 octaves
(test_mx4_cpu.grid_matrix): it is known exactly without calling dequantize, and a wrong scale
index cannot pass."""
import pytest
import torch

from p2p_llm_chat_go_amd import ops
from p2p_llm_chat_go_amd.ops._lib import KernelError
from test_mx4_cpu import grid_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


_CASES = {}


def _case(K, N):
    """(W fp32, Mx4Weight on the GPU) of one shape, built once."""
    if (K, N) not in _CASES:
        W = grid_matrix(N, K, K + N, e_lo=-9, e_hi=2)
        _CASES[(K, N)] = (W, ops.quantize_mxfp4(ops.tile_weight(W.to(torch.bfloat16))).to(DEV))
    return _CASES[(K, N)]


def _run(q, W, x, epi, norm, code=0):
    """(GPU output, fp32 reference) of one epilogue."""
    M, N = x.shape[0], W.shape[0]
    acc = x.float() @ W.t()
    if norm:
        acc = acc * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    xd = x.to(DEV)
    if epi == "store":
        return ops.skinny_gemm(q, xd, ops.EPI_STORE, norm=norm, waves=code), acc
    if epi == "f32":
        out = ops.skinny_gemm(q, xd, ops.EPI_F32, norm=norm, waves=code)
        assert out.dtype == torch.float32
        return out, acc
    if epi == "resid":
        h = (torch.randn(M, N) * acc.abs().mean()).to(torch.bfloat16)
        out = h.to(DEV)
        ops.skinny_gemm(q, xd, ops.EPI_RESID, norm=norm, out=out, waves=code)
        return out, h.float() + acc
    out = ops.skinny_gemm(q, xd, ops.EPI_SILU, norm=norm, waves=code)
    return out, torch.nn.functional.silu(acc[:, :N // 2]) * acc[:, N // 2:]


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("epi", ["store", "f32", "resid", "silu"])
@pytest.mark.parametrize("K,N", [(128, 48), (384, 64), (2048, 128)])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 40, 64, 100])
def test_mx4_gemm(M, K, N, epi, norm):
    if epi == "silu" and N % 32:
        N *= 2  # SwiGLU pairs whole 16-column groups: gate and up halves of three groups each
    W, q = _case(K, N)
    torch.manual_seed(M * 7 + K)
    x = torch.randn(M, K).to(torch.bfloat16)
    out, ref = _run(q, W, x, epi, norm)
    torch.cuda.synchronize()
    assert _rel(out.cpu(), ref) < 1e-2


@pytest.mark.parametrize("M", [5, 40])
@pytest.mark.parametrize("code", ops.MX4_CODES)
def test_mx4_gemm_launch_codes(M, code):
    K, N = 1024, 128
    W, q = _case(K, N)
    torch.manual_seed(code)
    x = torch.randn(M, K).to(torch.bfloat16)
    if not ops.mx4_code_ok(M, K, N, ops.EPI_STORE, True, code):
        with pytest.raises(KernelError):
            _run(q, W, x, "store", True, code)
        return
    out, ref = _run(q, W, x, "store", True, code)
    torch.cuda.synchronize()
    assert _rel(out.cpu(), ref) < 1e-2


@pytest.mark.parametrize("M", [1, 7, 100])  # 100: two row chunks
def test_mx4_qkv_rope(M):
    from p2p_llm_chat_go_amd.models.config import LLAMA31_8B, rope_table

    Hq, Hkv, K = 4, 2, 512
    N = (Hq + 2 * Hkv) * 128
    W = grid_matrix(N, K, M, e_lo=-9, e_hi=2)
    q4 = ops.quantize_mxfp4(ops.tile_weight(W.to(torch.bfloat16)))
    torch.manual_seed(M)
    x = torch.randn(M, K).to(torch.bfloat16)
    cs = rope_table(LLAMA31_8B, max_pos=2048)
    pos = torch.randint(0, 2000, (M,), dtype=torch.int32)
    slots = torch.randperm(4 * 64)[:M].to(torch.int32)
    outs = []
    for dev in ("cpu", DEV):  # CPU = the same fused op on the dequantized weight
        qo = torch.zeros(M, Hq * 128, dtype=torch.bfloat16, device=dev)
        kc = torch.zeros(4, Hkv, 64, 128, dtype=torch.bfloat16, device=dev)
        vc = torch.zeros_like(kc)
        ops.qkv_rope_gemm(q4.to(dev), x.to(dev), pos.to(dev), slots.to(dev), cs.to(dev), Hq, Hkv,
                          qo, kc, vc)
        outs.append([t.cpu() for t in (qo, kc, vc)])
    for a, b in zip(outs[1], outs[0]):
        assert _rel(a, b) < 1e-2


def test_engine_mxfp4_weights_decode_matches_dequantized_bf16():
    from p2p_llm_chat_go_amd.engine import Engine
    from p2p_llm_chat_go_amd.models.config import get_config
    from p2p_llm_chat_go_amd.models.weights import EngineWeights

    cfg = get_config("tiny-llama")
    e4 = Engine(cfg, weights=EngineWeights.random(cfg, DEV, seed=3), device=DEV, kv_pages=64,
                max_batch=4, weight_dtype="mxfp4")
    wd = EngineWeights.random(cfg, DEV, seed=3)
    for lw, l4 in zip(wd.layers, e4.weights.layers):
        for n in ("qkv", "o", "gate_up", "down"):
            assert isinstance(getattr(l4, n), ops.Mx4Weight)
            setattr(lw, n, getattr(l4, n).dequantize())
    wd.lm_head = e4.weights.lm_head.dequantize()  # the FP8 LM head of mxfp4 mode
    ed = Engine(cfg, weights=wd, device=DEV, kv_pages=64, max_batch=4)
    prompts = [[1, 5, 9, 200, 31], [7, 7, 3]]
    res = []
    for e in (e4, ed):
        bts = [e.kv.allocator.alloc(1) for _ in prompts]
        _first, logits = e.prefill(prompts, bts, return_logits=True)
        res.append(logits.float().cpu())
        for b in bts:
            e.kv.allocator.free(b)
    assert _rel(res[0], res[1]) < 2e-2
    assert len(e4.generate(prompts, max_new_tokens=8)[0].tokens) == 8
    assert e4.weights.nbytes() < ed.weights.nbytes()
