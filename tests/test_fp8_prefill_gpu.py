"""FP8 prefill GEMM (csrc/kernels/fp8_prefill_gemm.hip, M > 64) against fp32 on the CPU.
Neighbouring output channels carry scales a power of two apart, so a wrong scale index cannot
pass.  Relative Frobenius error < 1e-2, engine logits 2e-2, as for the skinny kernel's FP8 path."""
import pytest
import torch

from p2p_llm_chat_go_amd import ops
from p2p_llm_chat_go_amd.ops._lib import KernelError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CASES = {}
EPI = {"store": ops.EPI_STORE, "f32": ops.EPI_F32, "resid": ops.EPI_RESID, "silu": ops.EPI_SILU}


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _weight(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    W = 0.05 * torch.randn(N, K, generator=g) * torch.exp2((torch.arange(N) % 7 - 3).float())[:, None]
    return ops.quantize_fp8(ops.tile_weight(W.to(torch.bfloat16)))


def _case(K, N):
    """(dequantised fp32 W, Fp8Weight on the GPU) of one shape, built once."""
    if (K, N) not in _CASES:
        q = _weight(N, K, K + N)
        _CASES[(K, N)] = (q.dequantize_f32(), q.to(DEV))
    return _CASES[(K, N)]


def _run(q, W, x, epi, norm, code):
    """(GPU output, fp32 reference) of one epilogue."""
    M, N = x.shape[0], W.shape[0]
    acc = x.float() @ W.t()
    if norm:
        acc = acc * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    xd = x.to(DEV)
    if epi == "resid":
        h = (torch.randn(M, N) * acc.abs().mean()).to(torch.bfloat16)
        out = h.to(DEV)
        ops.skinny_gemm(q, xd, ops.EPI_RESID, norm=norm, out=out, waves=code)
        return out, h.float() + acc
    out = ops.skinny_gemm(q, xd, EPI[epi], norm=norm, waves=code)
    assert out.dtype == (torch.float32 if epi == "f32" else torch.bfloat16)
    if epi == "silu":
        return out, torch.nn.functional.silu(acc[:, :N // 2]) * acc[:, N // 2:]
    return out, acc


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("epi", list(EPI))
@pytest.mark.parametrize("K,N", [(128, 64), (384, 192), (1024, 256)])
@pytest.mark.parametrize("M", [65, 128, 129, 200, 300])
def test_fp8_prefill_gemm(M, K, N, epi, norm):
    assert ops.fp8_prefill_ok(M, K, N, EPI[epi], norm, 0)
    W, q = _case(K, N)
    torch.manual_seed(M * 7 + K)
    x = torch.randn(M, K).to(torch.bfloat16)
    out, ref = _run(q, W, x, epi, norm, ops.FP8_PREFILL_FLAG)  # the flag alone: default tile
    torch.cuda.synchronize()
    assert _rel(out.cpu(), ref) < 1e-2


@pytest.mark.parametrize("code", ops.FP8_PREFILL_CODES, ids=hex)
def test_fp8_prefill_tile_codes(code):
    M, K, N = 200, 1024, 192
    W, q = _case(K, N)
    torch.manual_seed(code & 0xff)
    x = torch.randn(M, K).to(torch.bfloat16)
    if not ops.fp8_prefill_ok(M, K, N, ops.EPI_STORE, True, code):
        with pytest.raises(KernelError):
            _run(q, W, x, "store", True, code)
        return
    out, ref = _run(q, W, x, "store", True, code)
    torch.cuda.synchronize()
    assert _rel(out.cpu(), ref) < 1e-2


@pytest.mark.parametrize("M", [100, 200])
def test_fp8_prefill_qkv_rope(M):
    from p2p_llm_chat_go_amd.models.config import LLAMA31_8B, rope_table

    Hq, Hkv, K = 4, 2, 512
    q8 = _weight((Hq + 2 * Hkv) * 128, K, M)
    torch.manual_seed(M)
    x = torch.randn(M, K).to(torch.bfloat16)
    cs = rope_table(LLAMA31_8B, max_pos=2048)
    pos = torch.randint(0, 2000, (M,), dtype=torch.int32)
    slots = torch.randperm(4 * 64)[:M].to(torch.int32)  # shuffled over four pages
    outs = []
    for dev in ("cpu", DEV):  # CPU = the same fused op on the dequantised weight
        qo = torch.zeros(M, Hq * 128, dtype=torch.bfloat16, device=dev)
        kc = torch.zeros(4, Hkv, 64, 128, dtype=torch.bfloat16, device=dev)
        vc = torch.zeros_like(kc)
        ops.qkv_rope_gemm(q8.to(dev), x.to(dev), pos.to(dev), slots.to(dev), cs.to(dev), Hq, Hkv,
                          qo, kc, vc, waves=ops.FP8_PREFILL_FLAG)
        outs.append([t.cpu() for t in (qo, kc, vc)])
    for a, b in zip(outs[1], outs[0]):
        assert _rel(a, b) < 1e-2


def test_fp8_prefill_deterministic_and_routed():
    W, q = _case(1024, 256)
    torch.manual_seed(300)
    x = torch.randn(300, 1024).to(torch.bfloat16)
    a, _ = _run(q, W, x, "store", True, ops.FP8_PREFILL_FLAG)
    b, _ = _run(q, W, x, "store", True, ops.FP8_PREFILL_FLAG)
    assert torch.equal(a, b)
    assert ops.fp8_route(64, 4096, 14336 * 2, ops.EPI_SILU, True) == "skinny"
    # profiles/fp8_prefill_gemm.jsonl: 8B gate_up at 512 rows
    assert ops.fp8_route(512, 4096, 14336 * 2, ops.EPI_SILU, True) == "prefill"


def test_engine_fp8_prefill_chunk_matches_dequantized_bf16():
    from p2p_llm_chat_go_amd.engine import Engine
    from p2p_llm_chat_go_amd.models.config import get_config
    from p2p_llm_chat_go_amd.models.weights import EngineWeights

    cfg = get_config("tiny-llama")
    e8 = Engine(cfg, weights=EngineWeights.random(cfg, DEV, seed=3), device=DEV, kv_pages=64,
                max_batch=4, weight_dtype="fp8")
    wd = EngineWeights.random(cfg, DEV, seed=3)
    for lw, l8 in zip(wd.layers, e8.weights.layers):
        for n in ("qkv", "o", "gate_up", "down"):
            setattr(lw, n, getattr(l8, n).dequantize())
    wd.lm_head = e8.weights.lm_head.dequantize()
    ed = Engine(cfg, weights=wd, device=DEV, kv_pages=64, max_batch=4)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(1, cfg.vocab, (n,), generator=g).tolist() for n in (70, 50, 30)]
    res = []
    for e in (e8, ed):  # 150 rows in one chunk, prefill graphs left on
        bts = [e.kv.allocator.alloc(2) for _ in prompts]
        _first, logits = e.prefill(prompts, bts, return_logits=True)
        res.append(logits.float().cpu())
        for b in bts:
            e.kv.allocator.free(b)
    assert _rel(res[0], res[1]) < 2e-2
    firsts = []
    for _ in range(4):  # the chunk shape is captured at its second use, then replayed
        bts = [e8.kv.allocator.alloc(2) for _ in prompts]
        firsts.append(e8.prefill(prompts, bts).cpu())
        for b in bts:
            e8.kv.allocator.free(b)
    assert e8._pgraphs
    assert all(torch.equal(f, firsts[0]) for f in firsts[1:])  # eager, capture, two replays
