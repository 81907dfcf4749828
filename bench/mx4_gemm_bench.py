"""Decode projections with bf16, FP8 and MXFP4 weights: us and effective TB/s (the format's own
weight bytes over time) at M = 1, 8, 64 for the llama3.1-8B and -70B shapes.  Cold weights:
each launch of a graph reads another copy, > 320 MB per cycle (past L2 and the 256 MB MALL).
Per format: the default launch (code 0) and the best of its autotune candidates.

    python bench/mx4_gemm_bench.py [--out profiles/mx4_gemm.jsonl] [--models 8b 70b]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_llm_chat_go_amd import ops  # noqa: E402
from p2p_llm_chat_go_amd.engine.autotune import _configs  # noqa: E402
from p2p_llm_chat_go_amd.ops import gemm as G  # noqa: E402
from kernel_bench import graph_time  # noqa: E402

SHAPES = {"8b": (4096, 14336, 6144), "70b": (8192, 28672, 10240)}  # hidden, ffn, qkv rows


def weights(fmt, N, K, n):
    """n distinct weights of one format; the values are random bits (timing only)."""
    def u8(*shape, lo=0, hi=256):
        return torch.randint(lo, hi, shape, device="cuda", dtype=torch.uint8)

    if fmt == "bf16":
        return [torch.randn(N // 16, K // 32, 64, 8, device="cuda").to(torch.bfloat16) for _ in range(n)]
    if fmt == "fp8":  # codes below 0x78: finite e4m3
        return [G.Fp8Weight(u8(N // 16, K // 32, 64, 8, hi=0x78), torch.ones(N, device="cuda"))
                for _ in range(n)]
    return [G.Mx4Weight(u8(N // 16, K // 128, 64, 16), u8(N // 16, K // 128, 16, 4, lo=120, hi=124))
            for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mx4_gemm.jsonl")
    ap.add_argument("--models", nargs="*", default=["8b", "70b"])
    a = ap.parse_args()
    bits = {"bf16": 16, "fp8": 8, "mx4": 4.25}
    with open(a.out, "w") as f:
        for model in a.models:
            H, F, QKV = SHAPES[model]
            for name, N, K, epi, norm in [("qkv", QKV, H, ops.EPI_STORE, True),
                                          ("o", H, H, ops.EPI_RESID, False),
                                          ("gate_up", 2 * F, H, ops.EPI_SILU, True),
                                          ("down", H, F, ops.EPI_RESID, False)]:
                for fmt in ("bf16", "fp8", "mx4"):
                    nbytes = N * K * bits[fmt] / 8
                    W = weights(fmt, N, K, max(1, min(40, int((320 << 20) // nbytes) + 1)))
                    for M in (1, 8, 64):
                        x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
                        out = torch.zeros(M, N // 2 if epi == ops.EPI_SILU else N, device="cuda",
                                          dtype=torch.bfloat16)
                        if fmt == "mx4":
                            codes = [c for c in G.MX4_CODES if G.mx4_code_ok(M, K, N, epi, norm, c)]
                        else:
                            codes = _configs(K, M)
                        t = {c: graph_time(lambda i: ops.skinny_gemm(W[i % len(W)], x, epi, norm=norm,
                                                                     out=out, waves=c))
                             for c in [0] + codes}
                        best = min(codes, key=t.get)
                        rec = {"model": model, "gemm": name, "N": N, "K": K, "M": M, "weights": fmt,
                               "copies": len(W), "us_default": round(t[0], 2),
                               "us_best": round(t[best], 2), "best_code": "w%d/U%d/NG%d" % (
                                   best & 0xff, (best >> 8) & 0xff, max(1, best >> 16)),
                               "TBps_best": round(nbytes / t[best] / 1e6, 3)}
                        print(json.dumps(rec), flush=True)
                        f.write(json.dumps(rec) + "\n")
                        f.flush()
                    del W


if __name__ == "__main__":
    main()
