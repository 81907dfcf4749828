"""FP8 projections above 64 rows: the prefill kernel (csrc/kernels/fp8_prefill_gemm.hip, every
tile code it serves) against the skinny kernel in 64-row chunks (what runs without it) and, for
information, the bf16 tiled kernel on a weight of the same shape.  The four projections of
llama3.1-8B and -70B at the prefill row buckets above 64, cold weights (each launch of a graph
reads another copy, > 320 MB per cycle), graph-replayed as in bench/mx4_prefill_bench.py.

Every path is timed twice, in two passes over all paths: ``us`` is the lower of the two and
``spread`` the largest relative difference between the passes of any path of that record.

    python bench/fp8_prefill_bench.py [--out profiles/fp8_prefill_gemm.jsonl] [--models 8b 70b]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_llm_chat_go_amd import ops  # noqa: E402
from p2p_llm_chat_go_amd.ops import gemm as G  # noqa: E402
from kernel_bench import graph_time  # noqa: E402
from mx4_gemm_bench import SHAPES, weights  # noqa: E402
from mx4_prefill_bench import ROWS, tile_name  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fp8_prefill_gemm.jsonl")
    ap.add_argument("--models", nargs="*", default=["8b", "70b"])
    ap.add_argument("--rows", type=int, nargs="*", default=list(ROWS))
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    route = G.fp8_route
    with open(a.out, "w") as f:
        for model in a.models:
            H, F, QKV = SHAPES[model]
            for name, N, K, epi, norm in [("qkv", QKV, H, ops.EPI_STORE, True),
                                          ("o", H, H, ops.EPI_RESID, False),
                                          ("gate_up", 2 * F, H, ops.EPI_SILU, True),
                                          ("down", H, F, ops.EPI_RESID, False)]:
                W = weights("fp8", N, K, max(1, min(40, int((320 << 20) // (N * K)) + 1)))
                Wb = weights("bf16", N, K, 2)
                for M in a.rows:
                    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
                    out = torch.zeros(M, N // 2 if epi == ops.EPI_SILU else N, device="cuda",
                                      dtype=torch.bfloat16)
                    paths = {tile_name(c): (W, c) for c in G.FP8_PREFILL_CODES
                             if G.fp8_prefill_ok(M, K, N, epi, norm, c)}
                    paths["chunked"] = (W, 0)
                    paths["bf16_tiled"] = (Wb, 0)
                    t = {k: [] for k in paths}
                    for _ in range(2):
                        for k, (ws, c) in paths.items():
                            # no launch code and no prefill route: the 64-row chunk loop
                            G.fp8_route = (lambda *s: "skinny") if k == "chunked" else route
                            t[k].append(graph_time(lambda i: ops.skinny_gemm(
                                ws[i % len(ws)], x, epi, norm=norm, out=out, waves=c), n_inner=a.inner))
                    G.fp8_route = route
                    us = {k: round(min(v), 2) for k, v in t.items()}
                    tiles = [k for k in us if k not in ("chunked", "bf16_tiled")]
                    best = min(tiles, key=us.get)
                    rec = {"model": model, "gemm": name, "N": N, "K": K, "M": M, "copies": len(W),
                           "us": us, "best_tile": best, "default_route": route(M, K, N, epi, norm),
                           "chunked_over_best": round(us["chunked"] / us[best], 3),
                           "spread": round(max(abs(v[0] - v[1]) / min(v) for v in t.values()), 3)}
                    print(json.dumps(rec), flush=True)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                del W, Wb


if __name__ == "__main__":
    main()
