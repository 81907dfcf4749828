"""FP8 KV cache flash prefill (kv_fp8_flash_prefill.hip, ops.flash_prefill_fp8) and the engine
route over it vs plain fp32 PyTorch references (run on an MI355X)."""
import functools
import math

import pytest
import torch

from p2p_llm_chat_go_amd import ops
from p2p_llm_chat_go_amd.ops import attention as A
from p2p_llm_chat_go_amd.ops import kv_fp8 as K8

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (start, n) per sequence: a start above 0 (a chunk continuing a cached prompt), page edges,
# a 1-token tile (a rider), tiles that end mid-page, more than one tile per sequence
LENS = [[(0, 5)], [(0, 37), (0, 16)], [(100, 70), (0, 300), (3, 1)], [(0, 600), (130, 257)]]


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _case(G, li):
    """Cache as tests/test_kv_fp8_gpu.py builds it: row magnitudes spread 20x (K) and 100x (V)
    inside a page, shuffled block tables, a null page with zero scales.  Returns the fp32
    reference and the device arguments of the flash and of the per-row kernel."""
    lens = LENS[li]
    g = torch.Generator().manual_seed(10 * G + li)
    Hkv, B = 2, len(lens)
    Hq, max_ctx = Hkv * G, max(s + n for s, n in lens)
    npg = (max_ctx + 63) // 64
    P = 1 + 4 * npg
    kf, vf = (torch.randn(P, Hkv, 64, 128, generator=g) * torch.logspace(-1, hi, 64)[:, None]
              for hi in (0.3, 1.0))
    kf[0], vf[0] = 0.0, 0.0
    (kc, ks), (vc, vs) = ops.quantize_kv_rows(kf), ops.quantize_kv_rows(vf)
    ks[0], vs[0] = 0.0, 0.0
    bt = (torch.rand(B, P - 1, generator=g).argsort(1)[:, :npg] + 1).to(torch.int32)
    seq, pos = [], []
    for b, (s0, n) in enumerate(lens):
        bt[b, (s0 + n + 63) // 64:] = 0  # entries past a context are the null page
        seq += [b] * n
        pos += list(range(s0, s0 + n))
    R = len(seq)
    q = torch.randn(R, Hq * 128, generator=g).to(torch.bfloat16)
    row_bt, ctx = torch.tensor(seq, dtype=torch.int32), torch.tensor(pos, dtype=torch.int32) + 1
    ref = K8.paged_attention_fp8_ref(q, kc, vc, ks, vs, bt, row_bt, ctx, Hq, Hkv,
                                     1 / math.sqrt(128), torch.empty(R, Hq * 128))
    qt = 256 // G
    tiles = torch.cat([ops.prefill_tiles(seq, pos, qt), torch.zeros(1, 4, dtype=torch.int32)])
    assert int(tiles[:, 1].sum()) == R and int(tiles[:, 1].max()) <= qt
    cache = tuple(x.to(DEV) for x in (q, kc, vc, ks, vs, bt))
    return ref, cache + (tiles.to(DEV), Hq, Hkv), cache + (row_bt.to(DEV), ctx.to(DEV), Hq, Hkv,
                                                           max_ctx), qt


def _flash(G, li):
    ref, fargs, _, qt = _case(G, li)
    out = torch.full(ref.shape, float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.flash_prefill_fp8(*fargs, out=out, qtile=qt)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("li", range(len(LENS)))
def test_flash_prefill_fp8(G, li):
    ref, _, rargs, _ = _case(G, li)
    out = _flash(G, li)
    assert not out.isnan().any()
    # both sides read the same codes and scales; only bf16 rounding of q, p and the output
    # differs (the bound of test_paged_attention_fp8 and test_flash_prefill)
    assert _rel(out.cpu(), ref) < 1e-2
    row = ops.paged_attention_fp8(*rargs)  # the decode kernel computes the same attention
    assert _rel(out, row) < 1e-2


def test_flash_prefill_fp8_is_deterministic():
    assert torch.equal(_flash(4, 2).view(torch.int16), _flash(4, 2).view(torch.int16))


def test_engine_kv_fp8_flash_matches_cpu_engine(monkeypatch):
    """A 200-token prompt in two chunks (128 + 72 rows) on the flash route, against the same
    engine on CPU tensors, as test_engine_kv_fp8_matches_cpu_engine compares them."""
    from p2p_llm_chat_go_amd.engine import Engine
    from p2p_llm_chat_go_amd.models import TINY_LLAMA as cfg
    from p2p_llm_chat_go_amd.models.reference import random_state_dict
    from p2p_llm_chat_go_amd.models.weights import EngineWeights

    monkeypatch.setattr(A, "FLASH_FP8_MIN_BLOCKS", 0)
    calls, real = [], ops.flash_prefill_fp8
    monkeypatch.setattr(ops, "flash_prefill_fp8",
                        lambda q, *a, **k: (calls.append(q.device.type), real(q, *a, **k))[1])
    sd = random_state_dict(cfg, seed=1)
    gpu, cpu = (Engine(cfg, weights=EngineWeights.from_state_dict(sd, cfg, d), device=d, kv_pages=16,
                       max_batch=2, max_prefill_tokens=128, kv_dtype="fp8") for d in (DEV, "cpu"))
    prompt = [1] + [(7 * i * i + 3 * i + 5) % 509 + 3 for i in range(199)]

    def logits(eng):
        pages = eng.kv.allocator.alloc(4)
        try:
            return eng.prefill([prompt], [pages], return_logits=True)[1][0].float().cpu()
        finally:
            eng.kv.allocator.free(pages)

    assert _rel(logits(gpu), logits(cpu)) < 3e-2
    assert calls.count("cuda") >= 2 * cfg.n_layers  # both chunks of the GPU engine, every layer
    got = gpu.generate([prompt], max_new_tokens=9, stop_on_eos=False)[0].tokens
    # the second run's prompt chunks replay their captured graphs
    assert len(got) == 9 and gpu.generate([prompt], max_new_tokens=9, stop_on_eos=False)[0].tokens == got
