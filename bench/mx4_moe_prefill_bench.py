"""Mixtral-8x7B expert GEMMs above 64 rows: the bf16 grouped launch, the MXFP4 window kernel
(csrc/kernels/mx4_moe_gemm.hip, forced by passing its default plan as an explicit code), the
MXFP4 grouped prefill kernel's default (csrc/kernels/mx4_moe_prefill_gemm.hip, forced by its
C entry point with code 0 whatever the route says) and every tile it serves: us per launch
at 96 .. 1024 tokens x top-2 over 8 experts (the seeded routing and the cold weight stacks of
bench/mx4_moe_bench.py).  Two passes; per record the spread between them and the minimum.

    python bench/mx4_moe_prefill_bench.py [--out profiles/mx4_moe_prefill_gemm.jsonl] [--tokens 96 ...]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_llm_chat_go_amd import ops  # noqa: E402
from p2p_llm_chat_go_amd.ops import _lib  # noqa: E402
from p2p_llm_chat_go_amd.ops import gemm as G  # noqa: E402
from p2p_llm_chat_go_amd.ops import moe as M  # noqa: E402
from kernel_bench import graph_time  # noqa: E402
from mx4_moe_bench import E, TOPK, H, F, routing, stacks  # noqa: E402

TOKENS = [96, 128, 192, 256, 512, 1024]


def window_default(R, K, N, epi, norm):
    """The window kernel's default plan above 32 rows (mx4_moe_plan) as an explicit code."""
    groups = N // (32 if epi == ops.EPI_SILU else 16)
    for ng in (4, 2, 1):
        for waves in (4, 2, 1):
            code = waves | 4 << 8 | ng << 16
            if groups % ng == 0 and (waves == 1 or K // 128 // waves >= 2) and \
                    M.mx4_grouped_ok(R, K, N, epi, norm, code):
                return code
    raise RuntimeError("no window plan")


def prefill_default(wt, cnt, rows, x, x_div, R, epi, out, norm, row_w):
    """The prefill kernel with code 0 (its own default tile), bypassing the route."""
    N, K = G.tiled_shape(wt[0])
    _lib.check(_lib.lib().p2p_mx4_grouped_prefill_gemm(
        wt.data.data_ptr(), wt.scale.data_ptr(), wt.data.stride(0), wt.scale.stride(0), E,
        cnt.data_ptr(), rows.data_ptr(), rows.stride(0), x_div, _lib.ptr(row_w), x.data_ptr(),
        x.stride(0), R, K, N, epi, int(norm), out.data_ptr(), out.stride(0), 1e-5, 0,
        _lib.stream_ptr(x.device)), "mx4_grouped_prefill_gemm")


def tile_name(c):
    return "%dx%d" % ((c & 0xf) * 64, ((c >> 4) & 0xf) * 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mx4_moe_prefill_gemm.jsonl")
    ap.add_argument("--tokens", type=int, nargs="*", default=TOKENS)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        for name, N, K, epi in [("w13", 2 * F, H, ops.EPI_SILU), ("w2", H, F, ops.EPI_STORE)]:
            silu = epi == ops.EPI_SILU
            W = {"bf16": stacks("bf16", N, K, 2), "mx4": stacks("mx4", N, K, 3)}
            for R in a.tokens:
                S = R * TOPK
                cnt, rows = routing(R)
                x = torch.randn(R if silu else S, K, device="cuda").to(torch.bfloat16)
                out = torch.zeros(S, N // 2 if silu else N, device="cuda", dtype=torch.bfloat16)
                row_w = None if silu else torch.rand(S, device="cuda")
                x_div = TOPK if silu else 1

                def timed(fmt, code=None):
                    ws = W[fmt]
                    if fmt == "mx4" and code is None:
                        return graph_time(lambda i: prefill_default(
                            ws[i % len(ws)], cnt, rows, x, x_div, R, epi, out, silu, row_w), n_inner=10)
                    kw = {"code": code} if fmt == "mx4" else {}
                    return graph_time(lambda i: M.grouped_gemm(
                        ws[i % len(ws)], cnt, rows, x, x_div, R, epi, out, norm=silu, row_w=row_w,
                        **kw), n_inner=10)

                tiles = [c for c in G.MX4_PREFILL_CODES if M.mx4_grouped_prefill_ok(R, K, N, epi, silu, c)]
                launches = [("bf16", 0), ("mx4", window_default(R, K, N, epi, silu)), ("mx4", None)] \
                    + [("mx4", c) for c in tiles]
                first = [timed(*l) for l in launches]
                second = [timed(*l) for l in launches]
                us = [min(p, q) for p, q in zip(first, second)]
                spread = max(abs(p - q) / min(p, q) for p, q in zip(first, second))
                by_tile = dict(zip(map(tile_name, tiles), us[3:]))
                best = min(by_tile, key=by_tile.get)
                rec = {"gemm": name, "N": N, "K": K, "tokens": R, "max_rows": R, "cnt": cnt.tolist(),
                       "us_bf16": round(us[0], 2), "us_mx4_window": round(us[1], 2),
                       "us_mx4_prefill_default": round(us[2], 2), "best_tile": best,
                       "us_mx4_prefill_best": round(by_tile[best], 2),
                       "window_over_prefill_default": round(us[1] / us[2], 3),
                       "bf16_over_prefill_default": round(us[0] / us[2], 3),
                       "default_over_best": round(us[2] / by_tile[best], 3),
                       "route": M.mx4_grouped_route(R, K, N, epi, silu), "spread": round(spread, 4),
                       "us_by_tile": {t: round(v, 2) for t, v in by_tile.items()}}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
                f.flush()
            del W
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
