"""Prompt-chunk attention over e4m3 pages: the MFMA flash prefill (ops.flash_prefill_fp8)
against the per-row kernel on the same rows (ops.paged_attention_fp8, ctx = pos + 1) and
against the bf16 flash prefill (ops.flash_prefill at its own ops.flash_tile width), us per
launch, at the llama3.1-8B (32/8 heads) and -70B (64/8) head shapes.  One sequence per chunk;
a chunk is (rows, first position): prompts from position 0 and two chunks that continue a
cached prompt.  Cold pages: every launch of a graph reads another set of pages, > 320 MB of
FP8 bytes per cycle (past L2 and the 256 MB MALL; the bf16 cycle is twice that).  The three
kernels alternate within the process, two passes each; the record keeps both and the largest
pass-to-pass spread.  The records back ops.attention.FLASH_FP8_MIN_BLOCKS.

    python bench/kv_fp8_flash_bench.py [--out profiles/kv_fp8_flash.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2p_llm_chat_go_amd import ops  # noqa: E402
from kernel_bench import graph_time  # noqa: E402

HEADS = {"8b": (32, 8), "70b": (64, 8)}
CHUNKS = [(128, 0), (256, 0), (512, 0), (1024, 0), (2048, 0), (8192, 0), (2048, 6144),
          (512, 31744)]
COLD_BYTES = 320 << 20
Hkv = 8


def page_sets(ctx):  # per cycle: the FP8 bytes of the sets exceed COLD_BYTES
    return COLD_BYTES // (Hkv * ctx * 132 * 2) + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/kv_fp8_flash.jsonl")
    ap.add_argument("--models", nargs="*", default=["8b", "70b"])
    ap.add_argument("--chunks", type=int, nargs="*", default=None,
                    help="indices into CHUNKS (default: all)")
    a = ap.parse_args()
    dev = "cuda"
    chunks = [CHUNKS[i] for i in a.chunks] if a.chunks else CHUNKS
    P = 1 + max(page_sets(p0 + R) * (-(-(p0 + R) // 64)) for R, p0 in chunks)
    # random finite values (timing only): bf16 pages, e4m3 codes below 0x78, scales of one
    kb, vb = (torch.randn(P, Hkv, 64, 128, device=dev).to(torch.bfloat16) for _ in range(2))
    k8, v8 = (torch.randint(0, 0x78, (P, Hkv, 64, 128), device=dev, dtype=torch.uint8)
              .view(torch.float8_e4m3fn) for _ in range(2))
    ks, vs = (torch.ones(P, Hkv, 64, device=dev) for _ in range(2))
    with open(a.out, "w") as f:
        for model in a.models:
            Hq, _ = HEADS[model]
            G = Hq // Hkv
            for R, p0 in chunks:
                ctx = p0 + R
                n, npg = page_sets(ctx), -(-ctx // 64)
                bt = (torch.randperm(P - 1, device=dev)[:n * npg] + 1).to(torch.int32)
                bt = bt.view(n, 1, npg)
                q = torch.randn(R, Hq * 128, device=dev).to(torch.bfloat16)
                out = torch.empty_like(q)
                pos = list(range(p0, ctx))
                qt8, qtb = 256 // G, ops.flash_tile(Hq, Hkv, R)
                t8 = ops.prefill_tiles([0] * R, pos, qt8).to(dev)
                tb = ops.prefill_tiles([0] * R, pos, qtb).to(dev)
                row_bt = torch.zeros(R, device=dev, dtype=torch.int32)
                cl = torch.tensor(pos, device=dev, dtype=torch.int32) + 1
                ws = ops.attn_workspace(R, Hq, ctx, dev)
                run = {
                    "flash_fp8": lambda i: ops.flash_prefill_fp8(
                        q, k8, v8, ks, vs, bt[i % n], t8, Hq, Hkv, out=out, qtile=qt8),
                    "row_fp8": lambda i: ops.paged_attention_fp8(
                        q, k8, v8, ks, vs, bt[i % n], row_bt, cl, Hq, Hkv, ctx, out=out,
                        workspace=ws),
                    "flash_bf16": lambda i: ops.flash_prefill(
                        q, kb, vb, bt[i % n], tb, Hq, Hkv, out=out, qtile=qtb)}
                t = {k: [] for k in run}
                for _ in range(2):  # alternate the kernels, two passes
                    for k, fn in run.items():
                        t[k].append(graph_time(fn, n_inner=max(n, 8), n_rep=3))
                best = {k: min(v) for k, v in t.items()}
                flops = 2 * 2 * Hq * 128 * sum(p + 1 for p in pos)  # the causal part only
                rec = {"model": model, "Hq": Hq, "Hkv": Hkv, "rows": R, "pos0": p0,
                       "blocks": t8.shape[0] * Hkv, "page_sets": n, "bf16_qtile": qtb,
                       **{"us_" + k: [round(x, 2) for x in v] for k, v in t.items()},
                       "spread": round(max(abs(v[0] - v[1]) / min(v) for v in t.values()), 4),
                       "flash_fp8_over_row_fp8": round(best["flash_fp8"] / best["row_fp8"], 3),
                       "flash_fp8_over_flash_bf16": round(best["flash_fp8"] / best["flash_bf16"], 3),
                       "TFLOPs_flash_fp8": round(flops / best["flash_fp8"] / 1e6, 1),
                       "TFLOPs_flash_bf16": round(flops / best["flash_bf16"] / 1e6, 1)}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
                f.flush()
                del ws


if __name__ == "__main__":
    main()
