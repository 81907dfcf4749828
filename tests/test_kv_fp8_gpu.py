"""FP8 KV cache kernels (kv_fp8_write.hip, kv_fp8_attention.hip) and the engine route over
them vs plain fp32 PyTorch references (run on an MI355X)."""
import math

import pytest
import torch

from p2p_llm_chat_go_amd import ops
from p2p_llm_chat_go_amd.ops import attention as A
from p2p_llm_chat_go_amd.ops import kv_fp8 as K8

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def kv_bound(x, s):
    """Half an e4m3 step of x / s (normal: 2^-4 relative; subnormal: 2^-10 absolute in code
    units), with 1 % for the fp32 rounding of s."""
    return 1.01 * torch.maximum(x.abs() * 2.0 ** -4, s[..., None] * 2.0 ** -10)


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (16, 2)])
@pytest.mark.parametrize("T", [1, 5, 70])
def test_rope_cache_fp8(Hq, Hkv, T):
    g = torch.Generator().manual_seed(100 * Hq + T)
    P, H = 8, Hq + 2 * Hkv
    qkv = (torch.randn(T, H * 128, generator=g) * torch.logspace(-2, 1, T)[:, None]).to(torch.bfloat16)
    qkv.view(T, H, 128)[0, -1, 3] = 300.0  # an outlier: the rest of that V row goes subnormal
    pos = torch.randint(0, 500, (T,), generator=g, dtype=torch.int32)
    ang = torch.arange(512)[:, None] * (10000.0 ** (-torch.arange(64) / 64.0))[None, :]
    cos_sin = torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()
    # token t -> page pg[t % 3] (shuffled), offset off[t // 3]: tokens 0 and 3 share a page
    pg, off = torch.randperm(P - 1, generator=g) + 1, torch.randperm(64, generator=g)
    t = torch.arange(T)
    slots = (pg[t % 3] * 64 + off[t // 3]).to(torch.int32)
    if T > 2:
        slots[2] = -1
    q_ref = torch.zeros(T, Hq * 128)
    k_ref, v_ref = torch.zeros(P, Hkv, 64, 128), torch.zeros(P, Hkv, 64, 128)
    A.rope_cache_ref(qkv.float(), pos, slots, cos_sin, Hq, Hkv, q_ref, k_ref, v_ref)

    perm = ops.rope_row_perm(H)
    q = torch.zeros(T, Hq * 128, device=DEV, dtype=torch.bfloat16)
    kc, vc = (torch.zeros(P, Hkv, 64, 128, device=DEV, dtype=F8) for _ in range(2))
    ks, vs = (torch.zeros(P, Hkv, 64, device=DEV) for _ in range(2))
    ops.rope_cache_fp8(qkv[:, perm].contiguous().to(DEV), pos.to(DEV), slots.to(DEV),
                       cos_sin.to(DEV), Hq, Hkv, q, kc, vc, ks, vs)
    torch.cuda.synchronize()
    assert bool(((q.cpu().float() - q_ref).abs() <= q_ref.abs() * 2.0 ** -8).all())  # bf16 rounding
    written = torch.zeros(P, 64, dtype=torch.bool)
    ok = slots >= 0
    written[(slots[ok] // 64).long(), (slots[ok] % 64).long()] = True
    for ref, codes, scale in ((k_ref, kc.cpu(), ks.cpu()), (v_ref, vc.cpu(), vs.cpu())):
        rows = written[:, None, :].expand(P, Hkv, 64)
        torch.testing.assert_close(scale[rows], ref.abs().amax(-1)[rows] / 448, rtol=1e-6, atol=0)
        assert not scale[~rows].any() and not codes.view(torch.uint8)[~rows].any()
        assert bool(((ops.dequantize_kv(codes, scale) - ref).abs() <= kv_bound(ref, scale)).all())


def _attention_case(G, ctxs, permute, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * G + len(ctxs))
    Hkv, B = 2, len(ctxs)
    Hq, max_ctx = Hkv * G, max(ctxs)
    npg = (max_ctx + 63) // 64
    P = 1 + 4 * npg  # every block-table row is its own shuffle of the pool's pages
    # row magnitudes vary 20x (K) and 100x (V) inside a page, so the scales matter
    kf, vf = (torch.randn(P, Hkv, 64, 128, generator=g) * torch.logspace(-1, hi, 64)[:, None]
              for hi in (0.3, 1.0))
    kf[0], vf[0] = 0.0, 0.0
    (kc, ks), (vc, vs) = ops.quantize_kv_rows(kf), ops.quantize_kv_rows(vf)
    ks[0], vs[0] = 0.0, 0.0  # the null page: zero codes with zero scales
    bt = (torch.rand(B + 1, P - 1, generator=g).argsort(1)[:, :npg] + 1).to(torch.int32)
    # block-table row B - r serves query row r when permuted, row r otherwise
    row_bt = (B - torch.arange(B)).to(torch.int32) if permute else None
    for r, c in enumerate(ctxs):  # entries past a context are the null page
        bt[B - r if permute else r, (c + 63) // 64:] = 0
    q = torch.randn(B, Hq * 128, generator=g).to(torch.bfloat16)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    ref = K8.paged_attention_fp8_ref(q, kc, vc, ks, vs, bt, row_bt, ctx, Hq, Hkv,
                                     1 / math.sqrt(128), torch.empty(B, Hq * 128))
    args = (q.to(DEV), kc.to(DEV), vc.to(DEV), ks.to(DEV), vs.to(DEV), bt.to(DEV),
            None if row_bt is None else row_bt.to(DEV), ctx.to(DEV), Hq, Hkv, max_ctx)
    return ref, args


# contexts 1 / 63, 64, 65 (page edges) / 255, 256, 257 (the chunk edge, where partials and the
# combine start) / 600 (a partly filled last chunk); batches of 1 and 3 rows
CTXS = [[1], [600], [63, 64, 65], [255, 256, 257], [600, 1, 257]]
# 127 / 128 rows x 2 kv heads: the row count from which a launch over more than one chunk
# runs one block per (row, kv head) that walks its row's chunks, with every context above
CTXS += [([1, 63, 64, 65, 255, 256, 257, 600] * 16)[:n] for n in (127, 128)]


@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("ctxs", CTXS)
@pytest.mark.parametrize("permute", [False, True])
def test_paged_attention_fp8(G, ctxs, permute):
    ref, args = _attention_case(G, ctxs, permute)
    out = ops.paged_attention_fp8(*args)
    torch.cuda.synchronize()
    # the bound of the bf16 paged_attention tests (tests/test_kernels_gpu.py:339): both sides
    # read the same codes and scales, only bf16 rounding of q, p and the output differs
    assert _rel(out.cpu(), ref) < 1e-2


def test_paged_attention_fp8_is_deterministic():
    _ref, args = _attention_case(4, [600, 1, 257], True, seed=7)
    a = ops.paged_attention_fp8(*args).clone()
    b = ops.paged_attention_fp8(*args)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))  # no atomics on this path


@pytest.mark.parametrize("weight_dtype", ["bf16", "mxfp4"])
def test_engine_kv_fp8_matches_cpu_engine(weight_dtype):
    """A 70-token prompt (crosses a page) and 8 greedy decode steps with graphs on, against
    the same engine on CPU tensors (reference ops, same quantisation rule), compared as
    tests/test_engine.py compares an engine with its oracle: prefill logits within 3e-2
    (_check_prefill_logits) and, teacher-forced, every token the reference's argmax unless
    the reference's own gap to it is a near-tie (_greedy_ok, margin 2e-2)."""
    from p2p_llm_chat_go_amd.engine import Engine
    from p2p_llm_chat_go_amd.models import TINY_LLAMA as cfg
    from p2p_llm_chat_go_amd.models.reference import random_state_dict
    from p2p_llm_chat_go_amd.models.weights import EngineWeights

    sd = random_state_dict(cfg, seed=1)
    gpu, cpu = (Engine(cfg, weights=EngineWeights.from_state_dict(sd, cfg, d), device=d, kv_pages=16,
                       max_batch=2, weight_dtype=weight_dtype, kv_dtype="fp8") for d in (DEV, "cpu"))
    prompt = [1] + [(7 * i * i + 3 * i + 5) % 509 + 3 for i in range(69)]

    def logits(eng, toks):
        pages = eng.kv.allocator.alloc(2)
        try:
            return eng.prefill([toks], [pages], return_logits=True)[1][0].float().cpu()
        finally:
            eng.kv.allocator.free(pages)

    a, b = logits(gpu, prompt), logits(cpu, prompt)
    assert _rel(a, b) < 3e-2
    got = gpu.generate([prompt], max_new_tokens=9, stop_on_eos=False)[0].tokens
    assert len(got) == 9
    # the second run's prompt chunk replays its captured graph (a shape is captured at its
    # second use): same tokens as the eager chunk
    assert gpu.generate([prompt], max_new_tokens=9, stop_on_eos=False)[0].tokens == got
    toks = list(prompt)
    for t in got:
        ref = logits(cpu, toks)
        if int(ref.argmax()) != t:
            assert float(ref.max() - ref[t]) < 2e-2 * float(ref.abs().max()), (t, len(toks))
        toks.append(t)
