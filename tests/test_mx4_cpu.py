"""MXFP4 weight format (ops.quantize_mxfp4 / Mx4Weight) and the CPU engine on it."""
import dataclasses

import pytest
import torch

from p2p_llm_chat_go_amd import ops
from p2p_llm_chat_go_amd.engine import Engine
from p2p_llm_chat_go_amd.models import TINY_LLAMA
from p2p_llm_chat_go_amd.models.weights import EngineWeights

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def grid_matrix(N, K, seed, e_lo=-8, e_hi=4):
    """Exactly representable W [N, K]: e2m1 grid values times a per-32-block power of two with
    exponents spread over [e_lo, e_hi]; every block holds a +-6, so its MX scale is determined."""
    g = torch.Generator().manual_seed(seed)
    v = GRID[torch.randint(0, 8, (N, K // 32, 32), generator=g)]
    v = v * (torch.randint(0, 2, v.shape, generator=g) * 2 - 1)
    v[:, :, 0] = 6.0 * (torch.randint(0, 2, (N, K // 32), generator=g) * 2 - 1)
    e = torch.randint(e_lo, e_hi + 1, (N, K // 32, 1), generator=g)
    return (v * torch.ldexp(torch.ones(()), e)).reshape(N, K)


def test_mxfp4_exact_round_trip():
    W = grid_matrix(32, 256, 0)
    q = ops.quantize_mxfp4(ops.tile_weight(W.to(torch.bfloat16)))
    assert q.data.shape == (2, 2, 64, 16) and q.scale.shape == (2, 2, 16, 4)
    assert q.data.dtype == q.scale.dtype == torch.uint8
    assert torch.equal(q.dequantize_f32(), W)
    assert torch.equal(ops.untile_weight(q.dequantize()).float(), W)
    assert ops.tiled_shape(q) == (32, 256)
    zero = ops.quantize_mxfp4(ops.tile_weight(torch.zeros(16, 128, dtype=torch.bfloat16)))
    assert (zero.scale == 127).all() and (zero.dequantize_f32() == 0).all()
    for bad in [(16, 96), (16, 192)]:  # K % 128 != 0
        with pytest.raises(AssertionError):
            ops.quantize_mxfp4(ops.tile_weight(torch.randn(*bad).to(torch.bfloat16)))


def test_mxfp4_error_bound_random_weights():
    torch.manual_seed(1)
    W = (torch.randn(64, 512) * 0.03).to(torch.bfloat16).float()
    Wd = ops.quantize_mxfp4(ops.tile_weight(W.to(torch.bfloat16))).dequantize_f32()
    # the OCP rule, written out: block scale 2^(floor(log2 amax) - 2); in units of the scale
    # the e2m1 spacing is 0.5 below 2, 1 below 4 and 2 up to 6, and values above 6 (up to
    # 8 = amax's bound) saturate at 6
    blk = W.reshape(64, 16, 32)
    scale = torch.exp2(torch.floor(torch.log2(blk.abs().amax(-1, keepdim=True))) - 2)
    a = blk.abs() / scale
    half_step = torch.where(a < 2, 0.25, torch.where(a < 4, 0.5, 1.0))
    bound = torch.where(a > 6, a - 6, half_step) * scale
    assert ((Wd.reshape(64, 16, 32) - blk).abs() <= bound).all()


def test_mxfp4_engine_cpu():
    w = EngineWeights.random(TINY_LLAMA, "cpu", seed=5)
    e4 = Engine(TINY_LLAMA, weights=w, device="cpu", kv_pages=64, max_batch=4,
                weight_dtype="mxfp4")
    assert all(isinstance(getattr(lw, n), ops.Mx4Weight)
               for lw in e4.weights.layers for n in ("qkv", "o", "gate_up", "down"))
    assert isinstance(e4.weights.lm_head, ops.Fp8Weight)
    assert isinstance(w.layers[0].qkv, torch.Tensor)  # the caller's store stays bf16
    res = e4.generate([[1, 5, 9, 200, 31], [7, 7, 3]], max_new_tokens=4)
    assert all(len(r.tokens) == 4 for r in res)

    def proj_bytes(ws):  # nbytes() of the store without embedding and LM head
        return dataclasses.replace(ws, embed=ws.embed[:0], lm_head=ws.embed[:0]).nbytes()

    assert proj_bytes(e4.weights) < 0.3 * proj_bytes(w)
    with pytest.raises(ValueError, match="tp_size"):
        Engine(TINY_LLAMA, device="cpu", kv_pages=8, weight_dtype="mxfp4", tp_size=2)
