"""MXFP4 grouped expert GEMM (csrc/kernels/mx4_moe_gemm.hip) against fp32 on the CPU.

The expert matrices are test_mx4_cpu.grid_matrix values (known exactly without dequantize);
the slot lists are cut from a seeded permutation, and every slot no list names must keep the
sentinel the output was filled with."""
import pytest
import torch

from p2p_llm_chat_go_amd import ops
from p2p_llm_chat_go_amd.ops import moe as M
from p2p_llm_chat_go_amd.ops._lib import KernelError
from test_mx4_cpu import grid_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = 4
SENTINEL = -768.0  # exact in bf16

_CASES = {}


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _case(K, N):
    """(W fp32 [E, N, K], stacked Mx4Weight on the GPU) of one shape, built once."""
    if (K, N) not in _CASES:
        W = torch.stack([grid_matrix(N, K, K + N + e, e_lo=-9, e_hi=2) for e in range(E)])
        q = ops.quantize_mxfp4(torch.stack([ops.tile_weight(w.to(torch.bfloat16)) for w in W]))
        _CASES[(K, N)] = (W, q.to(DEV))
    return _CASES[(K, N)]


def _run(K, N, counts, epi, code=0):
    """One grouped launch -> (output rows of the routed slots, their fp32 reference, the
    rows of every other slot)."""
    W, q = _case(K, N)
    g = torch.Generator().manual_seed(K + N + sum(counts))
    S = sum(counts) + 7  # 7 slots that no expert serves
    perm = torch.randperm(S, generator=g)
    max_rows = max(counts)
    rows = torch.full((E, max_rows), int(perm[-1]), dtype=torch.int32)  # padding: unrouted
    lists, at = [], 0
    for e, c in enumerate(counts):
        lists.append(perm[at:at + c])
        rows[e, :c] = lists[e].to(torch.int32)
        at += c
    cnt = torch.tensor(counts, dtype=torch.int32)
    silu = epi == ops.EPI_SILU
    x_div = 2 if silu else 1
    R = (S + x_div - 1) // x_div
    # rows of very different norms: a slot -> row mix-up in the RMSNorm shows
    x = (torch.randn(R, K, generator=g) * torch.linspace(0.2, 3.0, R)[:, None]).to(torch.bfloat16)
    row_w = None if silu else torch.rand(S, generator=g) + 0.1
    out = torch.full((S, N // 2 if silu else N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    M.grouped_gemm(q, cnt.to(DEV), rows.to(DEV), x.to(DEV), x_div, max_rows, epi, out, norm=silu,
                   row_w=None if silu else row_w.to(DEV), code=code)
    torch.cuda.synchronize()
    out = out.cpu()
    ref = torch.empty(at, out.shape[1])
    at = 0
    for e, sl in enumerate(lists):
        xf = x[sl // x_div].float()
        acc = xf @ W[e].t()
        if silu:
            acc = acc * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)
            acc = torch.nn.functional.silu(acc[:, :N // 2]) * acc[:, N // 2:]
        else:
            acc = acc * row_w[sl][:, None]
        ref[at:at + len(sl)] = acc
        at += len(sl)
    return out[perm[:at]], ref, out[perm[at:]]


COUNTS = [(1, 0, 0, 1), (5, 16, 17, 0), (64, 33, 1, 2), (70, 3, 0, 130)]


@pytest.mark.parametrize("epi", [ops.EPI_SILU, ops.EPI_STORE], ids=["w13_silu", "w2_store"])
@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("K,N", [(128, 64), (384, 96), (2048, 128)])
def test_mx4_grouped_gemm(K, N, counts, epi):
    got, ref, rest = _run(K, N, counts, epi)
    assert (rest == SENTINEL).all()
    assert _rel(got, ref) < 1e-2


@pytest.mark.parametrize("epi", [ops.EPI_SILU, ops.EPI_STORE], ids=["w13_silu", "w2_store"])
@pytest.mark.parametrize("code", ops.MX4_CODES)
def test_mx4_grouped_launch_codes(code, epi):
    K, N, counts = 1024, 128, (5, 40, 0, 17)
    if not M.mx4_grouped_ok(max(counts), K, N, epi, epi == ops.EPI_SILU, code):
        with pytest.raises(KernelError):
            _run(K, N, counts, epi, code)
        return
    got, ref, rest = _run(K, N, counts, epi, code)
    assert (rest == SENTINEL).all()
    assert _rel(got, ref) < 1e-2


def test_mx4_grouped_deterministic():
    a = _run(2048, 128, COUNTS[3], ops.EPI_SILU)[0]
    b = _run(2048, 128, COUNTS[3], ops.EPI_SILU)[0]
    assert torch.equal(a, b)


def test_engine_mxfp4_experts_match_dequantized_bf16():
    from p2p_llm_chat_go_amd.engine import Engine
    from p2p_llm_chat_go_amd.models.config import get_config
    from p2p_llm_chat_go_amd.models.weights import EngineWeights

    cfg = get_config("tiny-mixtral")
    # Routing margin of this seed, measured once on the CPU engine over the 60 routed rows of
    # this run (prefill and decode, both layers).  The random router (std 0.5) is peaked: the
    # first expert takes nearly all the mass, so the 2nd and 3rd router *probabilities* are
    # less than 0.02 apart on 42 rows (smallest gap 0.0000) at every seed tried -- a 0.02
    # probability gap does not exist for this store.  What holds for seed 6: the 2nd and 3rd
    # router *logits* are at least 0.357 apart on every row (the best of seeds 1..39), and
    # on the 42 rows the second expert's weight is at most 0.023.  Both engines multiply the
    # same weight values, so their logits differ by summation order only: no flip expected.
    seed = 6
    e4 = Engine(cfg, weights=EngineWeights.random(cfg, DEV, seed=seed), device=DEV, kv_pages=64,
                max_batch=4, weight_dtype="mxfp4")
    wd = EngineWeights.random(cfg, DEV, seed=seed)
    for lw, l4 in zip(wd.layers, e4.weights.layers):
        for n in ("qkv", "o", "w13", "w2"):
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
    assert all(len(r.tokens) == 8 for r in e4.generate(prompts, max_new_tokens=8))
