"""FP8 KV cache on CPU tensors: the reference quantiser, the cache accounting and the
engine plumbing (the GPU kernels: tests/test_kv_fp8_gpu.py)."""
import pytest
import torch

from p2p_llm_chat_go_amd import ops
from p2p_llm_chat_go_amd.engine import Engine
from p2p_llm_chat_go_amd.engine.kv_cache import KVCache
from p2p_llm_chat_go_amd.models import LLAMA31_8B, TINY_LLAMA


def kv_bound(x, s):
    """Half an e4m3 step of x / s (normal: 2^-4 relative; subnormal: 2^-10 absolute in code
    units), with 1 % for the fp32 rounding of s."""
    return 1.01 * torch.maximum(x.abs() * 2.0 ** -4, s[..., None] * 2.0 ** -10)


def test_quantiser_round_trip():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 128, generator=g) * torch.logspace(-3, 3, 64)[:, None]
    x[5] = 0.0
    x[9, 77] = 3e4  # one outlier pushes the rest of the row into the subnormal codes
    codes, s = ops.quantize_kv_rows(x)
    deq = ops.dequantize_kv(codes, s)
    assert codes.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    assert bool(((deq - x).abs() <= kv_bound(x, s)).all())
    assert s[5] == 1.0 and not deq[5].any()
    big = x.abs().argmax(-1, keepdim=True)
    torch.testing.assert_close(deq.gather(1, big), x.gather(1, big), rtol=1e-6, atol=0)


def test_cache_accounting():
    cfg = LLAMA31_8B
    assert KVCache.bytes_per_page(cfg, kv_dtype="fp8") == 2 * cfg.n_layers * cfg.n_kv_heads * 64 * 132
    tiny = TINY_LLAMA
    a = KVCache.from_free_memory(tiny, "cpu")
    b = KVCache.from_free_memory(tiny, "cpu", kv_dtype="fp8")
    assert b.num_pages >= 1.9 * a.num_pages
    k, v, ks, vs = b.layer_fp8(1)
    assert k.dtype == torch.float8_e4m3fn and k.shape == (b.num_pages, 1, 64, 128)
    assert ks.shape == (b.num_pages, 1, 64) and vs.dtype == torch.float32
    with pytest.raises(TypeError):
        b.layer(0)


def test_tiny_engine_generates_and_bad_dtype_raises():
    eng = Engine(TINY_LLAMA, device="cpu", seed=3, kv_pages=16, max_batch=2, kv_dtype="fp8")
    prompts = [[1, 5, 9, 33, 100, 7], list(range(3, 73))]  # the second crosses a page
    out = eng.generate(prompts, max_new_tokens=4, stop_on_eos=False)
    assert [len(r.tokens) for r in out] == [4, 4]
    # 6 + 70 prompt rows and 3 + 3 decode rows were written, per layer and kv head; the null
    # page was not
    assert int((eng.kv.k_scale > 0).sum()) == int((eng.kv.v_scale > 0).sum()) == 82 * 2
    assert not eng.kv.k_scale[:, 0].any() and not eng.kv.k.view(torch.uint8)[:, 0].any()
    with pytest.raises(ValueError):
        Engine(TINY_LLAMA, device="cpu", kv_pages=8, kv_dtype="int3")
