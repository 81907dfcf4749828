"""Stacked (per-expert) MXFP4 weights and the CPU Mixtral engine on 4-bit experts."""
import dataclasses

import torch

from p2p_llm_chat_go_amd import ops
from p2p_llm_chat_go_amd.engine import Engine
from p2p_llm_chat_go_amd.models import TINY_MIXTRAL
from p2p_llm_chat_go_amd.models.weights import EngineWeights
from test_mx4_cpu import grid_matrix


def test_mxfp4_stack_round_trip():
    Ws = [grid_matrix(32, 256, 10 + e) for e in range(3)]
    q = ops.quantize_mxfp4(torch.stack([ops.tile_weight(W.to(torch.bfloat16)) for W in Ws]))
    assert q.data.shape == (3, 2, 2, 64, 16) and q.scale.shape == (3, 2, 2, 16, 4)
    assert q.data.dtype == q.scale.dtype == torch.uint8
    assert q.shape == (3, 2, 8, 64, 8)
    for e, W in enumerate(Ws):
        assert isinstance(q[e], ops.Mx4Weight) and ops.tiled_shape(q[e]) == (32, 256)
        assert torch.equal(q[e].dequantize_f32(), W)
    assert torch.equal(q.dequantize_f32(), torch.stack(Ws))
    assert torch.equal(q.dequantize()[1], ops.tile_weight(Ws[1].to(torch.bfloat16)))
    assert q.nbytes() == 3 * (32 * 256 // 2 + 32 * 256 // 32)


def test_mxfp4_moe_engine_cpu():
    w = EngineWeights.random(TINY_MIXTRAL, "cpu", seed=5)
    e4 = Engine(TINY_MIXTRAL, weights=w, device="cpu", kv_pages=64, max_batch=4,
                weight_dtype="mxfp4")
    assert all(isinstance(getattr(lw, n), ops.Mx4Weight)
               for lw in e4.weights.layers for n in ("qkv", "o", "w13", "w2"))
    assert e4.weights.layers[0].w13.shape == w.layers[0].w13.shape
    assert isinstance(w.layers[0].w13, torch.Tensor)  # the caller's store stays bf16
    res = e4.generate([[1, 5, 9, 200, 31], [7, 7, 3]], max_new_tokens=4)
    assert all(len(r.tokens) == 4 for r in res)

    def proj_bytes(ws):  # nbytes() of the store without embedding and LM head
        return dataclasses.replace(ws, embed=ws.embed[:0], lm_head=ws.embed[:0]).nbytes()

    assert proj_bytes(e4.weights) < 0.3 * proj_bytes(w)
