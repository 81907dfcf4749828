"""Paged decode attention on bf16 pages (ops.paged_attention) against e4m3 pages
(ops.paged_attention_fp8): us per launch and the achieved bytes/s of each kernel's own KV
bytes, at the llama3.1-8B (32/8 heads) and -70B (64/8) head shapes, 1 and 8 rows, contexts
256 .. 32K.  Cold cache: every launch of a graph reads another set of pages, > 320 MB of the
FP8 kernel's bytes per cycle (past L2 and the 256 MB MALL; the bf16 cycle is twice that).
The two kernels alternate within the process, two passes each; the record keeps both and the
larger pass-to-pass spread.

    python bench/kv_fp8_attn_bench.py [--out profiles/kv_fp8_attn.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_llm_chat_go_amd import ops  # noqa: E402
from kernel_bench import graph_time  # noqa: E402

HEADS = {"8b": (32, 8), "70b": (64, 8)}
COLD_BYTES = 320 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/kv_fp8_attn.jsonl")
    ap.add_argument("--models", nargs="*", default=["8b", "70b"])
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--ctx", type=int, nargs="*", default=[256, 2048, 8192, 32768])
    a = ap.parse_args()
    dev = "cuda"
    Hkv = 8

    def launches(R, ctx):  # page sets per cycle: the FP8 bytes of a cycle exceed COLD_BYTES
        return COLD_BYTES // (R * Hkv * ctx * 132 * 2) + 2

    P = 1 + max(launches(R, c) * R * (c // 64) for R in a.rows for c in a.ctx)
    # random finite values (timing only): bf16 pages, e4m3 codes below 0x78, scales of one
    kb, vb = (torch.randn(P, Hkv, 64, 128, device=dev).to(torch.bfloat16) for _ in range(2))
    k8, v8 = (torch.randint(0, 0x78, (P, Hkv, 64, 128), device=dev, dtype=torch.uint8)
              .view(torch.float8_e4m3fn) for _ in range(2))
    ks, vs = (torch.ones(P, Hkv, 64, device=dev) for _ in range(2))
    with open(a.out, "w") as f:
        for model in a.models:
            Hq, _ = HEADS[model]
            for R in a.rows:
                for ctx in a.ctx:
                    n, npg = launches(R, ctx), ctx // 64
                    bt = (torch.randperm(P - 1, device=dev)[:n * R * npg] + 1).to(torch.int32)
                    bt = bt.view(n, R, npg)
                    q = torch.randn(R, Hq * 128, device=dev).to(torch.bfloat16)
                    out = torch.empty_like(q)
                    cl = torch.full((R,), ctx, device=dev, dtype=torch.int32)
                    ws = ops.attn_workspace(R, Hq, ctx, dev)
                    run = {
                        "bf16": lambda i: ops.paged_attention(q, kb, vb, bt[i % n], None, cl, Hq,
                                                              Hkv, ctx, out=out, workspace=ws),
                        "fp8": lambda i: ops.paged_attention_fp8(q, k8, v8, ks, vs, bt[i % n], None,
                                                                 cl, Hq, Hkv, ctx, out=out,
                                                                 workspace=ws)}
                    t = {k: [] for k in run}
                    for _ in range(2):  # alternate the kernels, two passes
                        for k, fn in run.items():
                            t[k].append(graph_time(fn, n_inner=max(n, 8)))
                    nbytes = {"bf16": R * Hkv * ctx * 256 * 2, "fp8": R * Hkv * ctx * 132 * 2}
                    best = {k: min(v) for k, v in t.items()}
                    rec = {"model": model, "Hq": Hq, "Hkv": Hkv, "rows": R, "ctx": ctx,
                           "page_sets": n,
                           "us_bf16": [round(x, 2) for x in t["bf16"]],
                           "us_fp8": [round(x, 2) for x in t["fp8"]],
                           "spread": round(max(abs(v[0] - v[1]) / min(v) for v in t.values()), 4),
                           "fp8_over_bf16_time": round(best["fp8"] / best["bf16"], 3),
                           "TBps_bf16": round(nbytes["bf16"] / best["bf16"] / 1e6, 3),
                           "TBps_fp8": round(nbytes["fp8"] / best["fp8"] / 1e6, 3)}
                    print(json.dumps(rec), flush=True)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
