"""Mixtral-8x7B expert GEMMs, bf16 grouped launch (skinny / LDS-tiled grouped kernels) against the
MXFP4 grouped kernel (csrc/kernels/mx4_moe_gemm.hip): us per launch for seven routing patterns,
built directly as cnt / rows from a seeded top-2 draw.  Cold weights: launch i of a graph reads
copy i of the stack (two bf16 / three MXFP4 copies: every launch reads more bytes than L2 and
the 256 MB MALL hold before a copy comes round again).  Per pattern: the bf16 launch, the MXFP4
default (code 0), the best served launch code, and the spread of a second pass over those three.

    python bench/mx4_moe_bench.py [--out profiles/mx4_moe_gemm.jsonl] [--patterns 1 8 ...]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_llm_chat_go_amd import ops  # noqa: E402
from p2p_llm_chat_go_amd.ops import gemm as G  # noqa: E402
from p2p_llm_chat_go_amd.ops import moe as M  # noqa: E402
from kernel_bench import graph_time  # noqa: E402

E, TOPK, H, F = 8, 2, 4096, 14336
# tokens of the pattern: 1 row x top-2, decode batches, a 64-row chunk, prompts
PATTERNS = {"1": 1, "8": 8, "32": 32, "64": 64, "44": 44, "256": 256, "1024": 1024}


def routing(R, seed=0):
    """cnt [E], rows [E, R] of R tokens that each draw two distinct experts (slot = 2 r + k)."""
    g = torch.Generator().manual_seed(seed + R)
    ids = torch.stack([torch.randperm(E, generator=g)[:TOPK] for _ in range(R)]).reshape(-1)
    cnt = torch.zeros(E, dtype=torch.int32)
    rows = torch.zeros(E, R, dtype=torch.int32)
    for s, e in enumerate(ids.tolist()):
        rows[e, cnt[e]] = s
        cnt[e] += 1
    return cnt.cuda(), rows.cuda()


def stacks(fmt, N, K, n):
    """n expert stacks of one format; the values are random bits (timing only)."""
    if fmt == "bf16":
        return [torch.empty(E, N // 16, K // 32, 64, 8, device="cuda", dtype=torch.bfloat16).normal_(0, 0.02)
                for _ in range(n)]
    return [G.Mx4Weight(torch.randint(0, 256, (E, N // 16, K // 128, 64, 16), device="cuda", dtype=torch.uint8),
                        torch.randint(120, 124, (E, N // 16, K // 128, 16, 4), device="cuda", dtype=torch.uint8))
            for _ in range(n)]


def code_name(c):
    return "w%d/U%d/NG%d" % (c & 0xff, (c >> 8) & 0xff, c >> 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mx4_moe_gemm.jsonl")
    ap.add_argument("--patterns", nargs="*", default=list(PATTERNS))
    a = ap.parse_args()
    with open(a.out, "w") as f:
        for name, N, K, epi in [("w13", 2 * F, H, ops.EPI_SILU), ("w2", H, F, ops.EPI_STORE)]:
            silu = epi == ops.EPI_SILU
            W = {"bf16": stacks("bf16", N, K, 2), "mx4": stacks("mx4", N, K, 3)}
            for pat in a.patterns:
                R = PATTERNS[pat]
                S = R * TOPK
                cnt, rows = routing(R)
                x = torch.randn(R if silu else S, K, device="cuda").to(torch.bfloat16)
                out = torch.zeros(S, N // 2 if silu else N, device="cuda", dtype=torch.bfloat16)
                row_w = None if silu else torch.rand(S, device="cuda")
                inner = 40 if R <= 64 else 10

                def timed(fmt, code):
                    ws = W[fmt]
                    kw = {"code": code} if fmt == "mx4" else {}
                    return graph_time(lambda i: M.grouped_gemm(
                        ws[i % len(ws)], cnt, rows, x, TOPK if silu else 1, R, epi, out, norm=silu,
                        row_w=row_w, **kw), n_inner=inner)

                codes = [c for c in G.MX4_CODES if M.mx4_grouped_ok(R, K, N, epi, silu, c)]
                t = {c: timed("mx4", c) for c in [0] + codes}
                best = min(codes, key=t.get)
                first = [timed("bf16", 0), t[0], t[best]]
                second = [timed("bf16", 0), timed("mx4", 0), timed("mx4", best)]
                spread = max(abs(p - q) / min(p, q) for p, q in zip(first, second))
                us = [min(p, q) for p, q in zip(first, second)]
                rec = {"gemm": name, "N": N, "K": K, "tokens": R, "max_rows": R,
                       "cnt": cnt.tolist(), "us_bf16": round(us[0], 2),
                       "us_mx4_default": round(us[1], 2), "us_mx4_best": round(us[2], 2),
                       "best_code": code_name(best), "bf16_over_mx4_default": round(us[0] / us[1], 3),
                       "spread": round(spread, 4),
                       "us_by_code": {code_name(c): round(t[c], 2) for c in codes}}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
                f.flush()
            del W
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
